// Comparison vectors (replaces gammas.py:65-124 evaluating the CASE templates of
// case_statements.py:62-277 with the jar's jaro_winkler_sim and Spark's levenshtein).
//
// Every comparison column is a small program of WHEN branches; each branch is an RPN predicate
// over SQL three-valued logic (NULL = branch not taken).  The program is uniform across a wave,
// so instruction fetch and dispatch are scalar; only the string work diverges.
//
// One lane per pair diverges badly if a wave must wait for its slowest lane's Jaro-Winkler or
// Levenshtein, so the evaluation is split:
//   1. filter pass (one lane per pair): NULL tests, equality (hash first), numeric tests and
//      *bounds* for the string similarities -- a Jaro-Winkler upper bound and a Levenshtein
//      lower / upper bound from 32-byte per-row metadata (lengths, hash, bucket sketch).  A
//      fourth truth value, UNDECIDED, propagates through AND / OR / NOT; a column whose WHEN
//      sequence is decided gets its level here, the others are appended (wave-aggregated) to
//      that column's work list.
//   2. exact pass (one lane per listed (pair, column)): the full interpreter with the exact
//      similarities computed from registers: match masks from per-row bit-planes (8 planes of
//      Latin-1 units, <= 64 units), Levenshtein after stripping the common prefix / suffix,
//      32-bit masks when the (trimmed) pattern fits.  Strings beyond 64 units, and surrogate
//      strings under Levenshtein, go to
//   3. the global-memory pass (two-row DP / flag words in scratch, any length up to SLOW_LIMIT).
// The filter pass writes each pair's code = Σ_k (γ_k + 1) · Π_{j<k}(L_j + 1) over the columns it
// decided (uint16 when the pattern space fits, else uint32); passes 2 and 3 add the rest in place.
// Bounds are exact decisions (never approximations), so the result is the exact evaluation.
//
// This unit holds the host side -- planner, windows, settlement, C entry points -- with the interpreter's filter
// kernel and the row-image kernels; the template filter is spk_filter.hip, passes 2 and 3 spk_exact.hip, the
// interpreter's device functions spk_interp.h (interfaces in spk_gamma.h).
#include <chrono>
#include <cstdio>
#include <algorithm>
#include <cstring>
#include <type_traits>
#include <cmath>

#include "spk_gamma.h"
#include "spk_interp.h"

namespace spk {

// rows_img: the image's row capacity (its chunk stride); rows [0, n) are filled.
__global__ void k_build_image(int64_t n, const ColDesc *__restrict__ cols, const SimpleCol *__restrict__ simple,
                              int n_simple, uint8_t *__restrict__ img, int64_t rows_img) {
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n) return;
    for (int j = 0; j < n_simple; ++j) {
        const SimpleCol &sc = simple[j];
        const ColDesc &c = cols[sc.col];
        if (sc.cls == SC_NUM) {
            const bool ok = c.valid[row] != 0;
            *reinterpret_cast<double *>(img + img_at(rows_img, row, sc.off)) = ok ? c.val[row] : 0.0;
            *reinterpret_cast<uint2 *>(img + img_at(rows_img, row, sc.off + 8)) = make_uint2(ok ? 1u : 0u, 0u);
            continue;
        }
        if (sc.cls == SC_LEV && sc.pos) {
            *reinterpret_cast<uint4 *>(img + img_at(rows_img, row, sc.off)) = c.pos[row];
            continue;
        }
        const RecMeta m = c.meta[row];
        uint32_t lens = LENS_NULL;
        if (m.len16 >= 0) {
            const int l16 = m.len16 < LEN_SAT ? m.len16 : LEN_SAT;
            const int lcp = meta_cplen(m) < LEN_SAT ? meta_cplen(m) : LEN_SAT;
            lens = (uint32_t)l16 | ((uint32_t)lcp << 16);
        }
        if (sc.eq4) {  // half of a JW gap: the id alone (NULL = all ones; ids are dense, < 2^32 - 1)
            *reinterpret_cast<uint32_t *>(img + img_at(rows_img, row, sc.off)) = m.len16 < 0 ? 0xFFFFFFFFu : m.key;
            continue;
        }
        *reinterpret_cast<uint2 *>(img + img_at(rows_img, row, sc.off)) = make_uint2(m.key, lens);
        if (sc.cls != SC_EQ) *reinterpret_cast<uint64_t *>(img + img_at(rows_img, row, sc.off + 8)) = m.sketch;
        if (sc.cls == SC_JW) *reinterpret_cast<uint64_t *>(img + img_at(rows_img, row, sc.off2)) = m.head;
    }
}

// Filter pass, every other column through the interpreter: adds to code[p].
__global__ __launch_bounds__(F_THREADS) void k_gamma_filter(GammaArgs A) {
    __shared__ unsigned int s_cnt[MAX_SIMPLE];
    for (int i = threadIdx.x; i < A.n_complex; i += F_THREADS) s_cnt[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const Region R = my_region(A);
    for (int64_t base = R.r0 + (threadIdx.x & ~63); base < R.r1; base += F_THREADS) {  // wave-uniform
        const int64_t p = base + lane;
        const bool active = p < R.r1;
        int32_t x = 0, y = 0;
        if (active) {
            x = A.pl[p];
            y = A.pr[p];
        }
        uint32_t acc = 0;
        for (int i = 0; i < A.n_complex; ++i) {
            const int k = A.complex_k[i];
            bool undecided = false;
            if (active) {
                int level = 0;
                const int st = eval_column<M_FILTER>(A, k, x, y, level);
                if (st == ST_DONE) acc += (uint32_t)(level + 1) * (uint32_t)A.stride[k];
                else undecided = true;
            }
            wave_append(region_list(A, k, R), &s_cnt[i], undecided, (int32_t)p);
        }
        if (active) code_add(A, p, acc);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < A.n_complex; i += F_THREADS)
        A.region_count[(int64_t)A.complex_k[i] * A.n_regions + A.region_base + blockIdx.x] = s_cnt[i];
}

__global__ void k_codes_from_gammas(int64_t n, int K, const int8_t *__restrict__ g, const int64_t *__restrict__ stride,
                                    uint8_t *codes, int code_bytes) {
    int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    uint32_t acc = 0;
    for (int k = 0; k < K; ++k) acc += (uint32_t)(g[p * K + k] + 1) * (uint32_t)stride[k];
    if (code_bytes == 2) reinterpret_cast<uint16_t *>(codes)[p] = (uint16_t)acc;
    else reinterpret_cast<uint32_t *>(codes)[p] = acc;
}

__global__ void k_gammas_from_codes(int64_t start, int64_t n, int K, const uint8_t *codes, int code_bytes,
                                    const int64_t *__restrict__ stride, const int32_t *__restrict__ nlev,
                                    int8_t *__restrict__ out) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int64_t p = start + i;
    uint32_t c = code_bytes == 2 ? reinterpret_cast<const uint16_t *>(codes)[p] : reinterpret_cast<const uint32_t *>(codes)[p];
    for (int k = 0; k < K; ++k) out[i * K + k] = (int8_t)((c / (uint32_t)stride[k]) % (uint32_t)(nlev[k] + 1)) - 1;
}

static int set_pattern_space(spk_ctx *ctx, int K, const int32_t *nlev) {
    SPK_REQUIRE(K >= 1 && K <= 64, SPK_E_INVALID, "need 1..64 comparison columns");
    ctx->K = K;
    ctx->n_levels.assign(nlev, nlev + K);
    ctx->stride.assign(K, 1);
    int64_t s = 1;
    for (int k = 0; k < K; ++k) {
        SPK_REQUIRE(nlev[k] >= 1 && nlev[k] <= 126, SPK_E_INVALID, "num_levels out of range");
        ctx->stride[k] = s;
        s *= (int64_t)(nlev[k] + 1);
        // pattern indices and their count are int on the device (PatArgs::n_pat): 2^31 itself does not fit
        SPK_REQUIRE(s < (int64_t)1 << 31, SPK_E_LIMIT,
                    "comparison-vector pattern space reaches 2^31 (too many columns x levels)");
    }
    ctx->n_patterns = s;
    ctx->code_bytes = s <= 65536 ? 2 : 4;
    ctx->mpat_valid = false;
    return SPK_OK;
}

}  // namespace spk

using namespace spk;

std::vector<uint16_t> spk::utf8_to_utf16(const uint8_t *b, int64_t n, int32_t *ncp) {
    std::vector<uint16_t> out;
    int64_t i = 0;
    int32_t c = 0;
    while (i < n) {
        uint32_t c0 = b[i], cp;
        int len;
        if (c0 < 0x80) { cp = c0; len = 1; }
        else if (c0 < 0xE0) { cp = c0 & 0x1F; len = 2; }
        else if (c0 < 0xF0) { cp = c0 & 0x0F; len = 3; }
        else { cp = c0 & 0x07; len = 4; }
        for (int k = 1; k < len && i + k < n; ++k) cp = (cp << 6) | (b[i + k] & 0x3F);
        i += len;
        if (cp >= 0x10000) {
            cp -= 0x10000;
            out.push_back((uint16_t)(0xD800 + (cp >> 10)));
            out.push_back((uint16_t)(0xDC00 + (cp & 0x3FF)));
        } else {
            out.push_back((uint16_t)cp);
        }
        ++c;
    }
    *ncp = c;
    return out;
}

static bool host_cmp(double a, double b, int cmp) {
    switch (cmp) {
        case SPK_CMP_EQ: return a == b;
        case SPK_CMP_NE: return a != b;
        case SPK_CMP_LT: return a < b;
        case SPK_CMP_LE: return a <= b;
        case SPK_CMP_GT: return a > b;
        default: return a >= b;
    }
}

static int32_t clamp_i32(double v) { return (int32_t)std::max(-1073741824.0, std::min(1073741824.0, v)); }

// The filter's per-test decision parameters (SimpleCol.tflag / lev_a / jw_cf), so the device decides
// each test with compares and selects only.
static void prepare_tests(SimpleCol &s) {
    for (int i = 0; i < s.n_tests; ++i) {
        const int op = s.op[i], cmp = s.cmp[i];
        const double t = s.t[i];
        int32_t f = 0;
        if (op == SPK_OP_STR_CMP) f |= cmp == SPK_CMP_EQ ? TF_EQ : 0;
        if (op == SPK_OP_JW || op == SPK_OP_LEVRATIO) {
            f |= host_cmp(0.0, t, cmp) ? TF_ZERO : 0;
            f |= host_cmp(1.0, t, cmp) ? TF_ONE : 0;
        }
        s.lev_a[i] = 0;
        s.jw_cf[i] = 0.f;
        if (op == SPK_OP_LEV) {  // integer v: v cmp t as v >= A or v <= A
            switch (cmp) {
                case SPK_CMP_GT: f |= TF_GE; s.lev_a[i] = clamp_i32(std::floor(t) + 1.0); break;
                case SPK_CMP_GE: f |= TF_GE; s.lev_a[i] = clamp_i32(std::ceil(t)); break;
                case SPK_CMP_LT: s.lev_a[i] = clamp_i32(std::ceil(t) - 1.0); break;
                case SPK_CMP_LE: s.lev_a[i] = clamp_i32(std::floor(t)); break;
                default: f |= TF_EXACT; break;
            }
        }
        if (op == SPK_OP_JW) {
            // an fp32 upper bound hi (of a double value) proves `v > t` false iff hi <= t, i.e. hi <=
            // the largest float <= t; `v >= t` false iff hi < t, i.e. hi < the smallest float >= t
            float fl = (float)t;
            if ((double)fl > t) fl = std::nextafter(fl, -INFINITY);
            float fu = (float)t;
            if ((double)fu < t) fu = std::nextafter(fu, INFINITY);
            s.jw_cf[i] = cmp == SPK_CMP_GT ? std::nextafter(fl, INFINITY) : fu;
        }
        s.tflag[i] = f;
    }
}

// Level of a simple string column for two equal, non-NULL, non-empty strings: `=` holds, jw = 1.0,
// levenshtein = 0 and its ratio 0.0 (den > 0); the first test that holds decides.
static int32_t equal_level(const SimpleCol &s) {
    for (int i = 0; i < s.n_tests; ++i) {
        const int op = s.op[i], cmp = s.cmp[i];
        bool r;
        if (op == SPK_OP_STR_CMP) r = cmp == SPK_CMP_EQ;
        else if (op == SPK_OP_JW) r = host_cmp(1.0, s.t[i], cmp);
        else r = host_cmp(0.0, s.t[i], cmp);  // SPK_OP_LEV / SPK_OP_LEVRATIO
        if (r) return s.level[i];
    }
    return s.else_level;
}

// The pairs of one blocking rule are contiguous in the pair order; a rule whose key includes the
// plain term `l.c = r.c` on the raw columns column c was decoded from puts equal, non-NULL strings
// of c in every pair it emits (keys are byte-verified dense ids; NULL keys emit nothing).  The
// longest run of such pairs becomes the column's implied range (SimpleCol.imp_lo / imp_hi).
static void implied_equal(const spk_ctx *ctx, const Table &t0, const Table &t1, SimpleCol &sc) {
    sc.imp_lo = sc.imp_hi = 0;
    sc.eq_level = 0;
    if (sc.kind != SK_STR || !(sc.cls == SC_EQ || sc.cls == SC_JW || sc.cls == SC_LEV)) return;
    const Column *c0 = t0.cols[sc.col], *c1 = t1.cols[sc.col];
    if (!c0 || !c1 || !c0->src[0] || !c1->src[1] || c0->has_empty || c1->has_empty) return;
    int64_t lo = -1, hi = -1;
    for (size_t r = 0; r < ctx->pair_terms.size(); ++r) {
        bool imp = false;
        for (const KeyTerm &k : ctx->pair_terms[r]) imp = imp || (k.plain && k.src_l == c0->src[0] && k.src_r == c1->src[1]);
        if (!imp) continue;
        if (lo >= 0 && ctx->pair_rule_lo[r] == hi) hi = ctx->pair_rule_hi[r];  // adjacent rules merge
        else lo = ctx->pair_rule_lo[r], hi = ctx->pair_rule_hi[r];
        if (hi - lo > sc.imp_hi - sc.imp_lo) sc.imp_lo = lo, sc.imp_hi = hi;
    }
    sc.eq_level = equal_level(sc);
}

// Filter class of a simple column (see SimpleCol); SC_NONE leaves it to the interpreter.
static int32_t simple_class(const SimpleCol &s) {
    if (s.kind == SK_NUM) return SC_NUM;
    bool all_eq = true, all_jw = s.n_tests > 0, lev_ok = true;
    int n_lev = 0;
    for (int i = 0; i < s.n_tests; ++i) {
        const int op = s.op[i], cmp = s.cmp[i];
        all_eq = all_eq && op == SPK_OP_STR_CMP;
        all_jw = all_jw && op == SPK_OP_JW && (cmp == SPK_CMP_GT || cmp == SPK_CMP_GE);
        if (op == SPK_OP_LEV) {
            ++n_lev;
        } else if (op == SPK_OP_LEVRATIO) {
            ++n_lev;
            lev_ok = lev_ok && (cmp == SPK_CMP_LE || cmp == SPK_CMP_LT);
        } else if (op != SPK_OP_STR_CMP) {
            lev_ok = false;
        }
    }
    if (all_eq) return SC_EQ;
    if (all_jw) return SC_JW;
    if (lev_ok && n_lev > 0) return SC_LEV;
    return SC_NONE;
}

// Row-image offsets; returns the row stride (a multiple of 16), 0 when nothing uses the image.
// JW fields take 24 B at a 16-byte boundary (key, lens, sketch; head units at off + 16, the low half
// of the next chunk), LEV / NUM 16 B at a boundary, EQ in the 8-byte gaps JW leaves (an EQ column with
// dictionary ids takes 4 B there -- its id, two to a gap, so one head-chunk load serves a JW column and
// two equality columns -- one without ids the whole gap), then 8 B each at the end.
// Columns that do not fit in IMG_MAX bytes, or past the filter kernel's slots of their class
// (FJ_MAX ...), go to the interpreter (SC_NONE).
static int64_t layout_image(std::vector<SimpleCol> &simple) {
    int64_t off = 0;
    std::vector<int64_t> gaps;  // free 8-byte slots
    int nj = 0, nl = 0, nn = 0, ne = 0;
    for (SimpleCol &s : simple) {
        if (s.cls != SC_JW) continue;
        if (off + 32 > IMG_MAX || nj == FJ_MAX) {
            s.cls = SC_NONE;
            continue;
        }
        ++nj;
        s.off = (int32_t)off;
        s.off2 = (int32_t)(off + 16);
        gaps.push_back(off + 24);
        off += 32;
    }
    for (SimpleCol &s : simple) {
        if (s.cls != SC_LEV && s.cls != SC_NUM) continue;
        int &n = s.cls == SC_LEV ? nl : nn;
        if (off + 16 > IMG_MAX || n == (s.cls == SC_LEV ? FL_MAX : FN_MAX)) {
            s.cls = SC_NONE;
            continue;
        }
        ++n;
        s.off = (int32_t)off;
        off += 16;
    }
    std::vector<int> used(gaps.size(), 0);  // 4-byte halves taken in each gap
    for (SimpleCol &s : simple) s.eq4 = 0;
    for (int pass = 0; pass < 2; ++pass) {  // ids first (half gaps), then the others (whole gaps)
        for (SimpleCol &s : simple) {
            if (s.cls != SC_EQ || (pass == 0) != (s.has_ids != 0)) continue;
            if (ne == FE_MAX) {
                s.cls = SC_NONE;
                continue;
            }
            size_t g = 0;
            const int need = pass == 0 ? 1 : 2;
            while (g < gaps.size() && used[g] + need > 2) ++g;
            if (g < gaps.size()) {
                s.off = (int32_t)(gaps[g] + 4 * used[g]);
                s.eq4 = pass == 0 ? 1 : 0;
                used[g] += need;
                ++ne;
                continue;
            }
            if (off + 8 > IMG_MAX) {
                s.cls = SC_NONE;
                continue;
            }
            ++ne;
            s.off = (int32_t)off;
            off += 8;
        }
    }
    int64_t end = off;
    if (!gaps.empty() && used.back() == 0 && gaps.back() + 8 == off) end = off - 8;  // trailing unused JW gap
    return (end + 15) & ~(int64_t)15;
}

// Row image in a rule's view order: chunk c of view position v = chunk c of table row rows[v]; the
// same chunk stride (row capacity) as the table's image.
__global__ void k_view_image(int64_t nv, const int32_t *__restrict__ rows, int nq, const uint4 *__restrict__ src,
                             uint4 *__restrict__ dst, int64_t cap) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nv * nq) return;
    const int64_t v = i % nv, c = i / nv;
    dst[c * cap + v] = src[c * cap + rows[v]];
}

// View-ordered copies of the row images for rule 1's pairs (RuleView), rebuilt when the image or the
// pair set changes.  Returns false when there is no view to use.
struct ViewLaunch {
    const uint8_t *img0, *img1;
    const int32_t *rows0, *rows1;  // view position -> table row
    int64_t lo, hi;                // rule 1's pair ordinals
};

static int build_view_images(spk_ctx *ctx, const GammaArgs &A, int64_t stride, ViewLaunch *out, bool *ok) {
    *ok = false;
    if (stride <= 0 || A.n_simple == 0 || ctx->n_views < 1 || !A.img0) return SPK_OK;
    const int nq = (int)(stride / 16);
    const int r = 1;
    RuleView &v = ctx->views[r];
    for (int s = 0; s < 2; ++s) {
        const int64_t nv = (s == 0 || v.tri) ? v.nL : v.nR;
        const int32_t *rows = (s == 0 || v.tri) ? v.rowsL.p : v.rowsR.p;
        if (s == 1 && v.tri) {  // symmetric self-join: both sides index the same view
            out->img1 = out->img0;
            out->rows1 = out->rows0;
            continue;
        }
        const int64_t cap = s == 0 ? A.img_rows0 : A.img_rows1;
        const uint8_t *src = s == 0 ? A.img0 : A.img1;
        std::vector<int64_t> key = ctx->img_key[(s == 1 && A.img1 != A.img0) ? 1 : 0];
        key.push_back((int64_t)ctx->pairs_epoch);
        key.push_back(s);
        const bool fresh = ctx->vimg[r][s].p && ctx->vimg_key[r][s] == key;
        SPK_TRY(ctx->vimg[r][s].alloc((size_t)cap * (size_t)stride));
        if (!fresh && nv > 0) {
            k_view_image<<<(unsigned)((nv * nq + 255) / 256), 256, 0, ctx->stream>>>(
                nv, rows, nq, reinterpret_cast<const uint4 *>(src), reinterpret_cast<uint4 *>(ctx->vimg[r][s].p), cap);
            SPK_HIP(hipGetLastError());
        }
        ctx->vimg_key[r][s] = key;
        (s == 0 ? out->img0 : out->img1) = ctx->vimg[r][s].p;
        (s == 0 ? out->rows0 : out->rows1) = rows;
    }
    out->lo = v.pair_lo;
    out->hi = v.pair_hi;
    *ok = true;
    return SPK_OK;
}

// The image is a re-layout of the resident records for the current set of simple columns: it is
// rebuilt only when a table (or one of its columns) was replaced or the column layout changed.
static int build_images(spk_ctx *ctx, Table &t0, Table &t1, GammaArgs &A, int64_t stride,
                        const std::vector<SimpleCol> &simple) {
    A.img0 = A.img1 = nullptr;
    A.img_stride = stride;
    if (stride <= 0 || A.n_simple == 0) return SPK_OK;
    Table *ts[2] = {&t0, &t1};
    for (int s = 0; s < 2; ++s) {
        if (s == 1 && &t1 == &t0) {
            A.img1 = A.img0;
            A.img_rows1 = A.img_rows0;
            break;
        }
        Table &t = *ts[s];
        std::vector<int64_t> key = {(int64_t)t.version, t.n, stride};
        for (const SimpleCol &sc : simple) {
            key.push_back(sc.cls);
            key.push_back(sc.col);
            key.push_back(sc.off);
            key.push_back(sc.off2);
            key.push_back(sc.eq4);
            key.push_back(sc.pos);
        }
        const bool fresh = ctx->img[s].p && ctx->img_key[s] == key;
        SPK_TRY(ctx->img[s].alloc((size_t)(t.n + 1) * (size_t)stride));
        ctx->img_key[s] = key;
        if (t.n > 0 && !fresh) {
            k_build_image<<<(unsigned)((t.n + 255) / 256), 256, 0, ctx->stream>>>(t.n, t.d_desc.p, A.simple, A.n_simple,
                                                                                 ctx->img[s].p, t.n + 1);
            SPK_HIP(hipGetLastError());
        }
        (s == 0 ? A.img0 : A.img1) = ctx->img[s].p;
        (s == 0 ? A.img_rows0 : A.img_rows1) = t.n + 1;
    }
    return SPK_OK;
}

static bool classify_simple(int k, const spk_column_program &prog, const int32_t *wf, const int32_t *wn,
                            const int32_t *wl, const spk_instr *instr, const spk_operand *ops, const Table &t0,
                            const Table &t1, const std::vector<int64_t> &stride, SimpleCol *out) {
    if (prog.n_when < 1 || prog.n_when - 1 > MAX_TESTS) return false;
    const int w0 = prog.first_when;
    if (wn[w0] != 3) return false;
    const spk_instr *n = instr + wf[w0];
    if (n[0].op != SPK_OP_ISNULL || n[1].op != SPK_OP_ISNULL || n[2].op != SPK_OP_OR) return false;
    auto plain = [&](int i, int side) {
        const spk_operand &o = ops[i];
        return o.kind == 0 && o.side == side && o.lit < 0 && !o.has_num_default && o.substr_start == 0;
    };
    int a = n[0].a, b = n[1].a;
    if (plain(b, 0) && plain(a, 1)) std::swap(a, b);
    if (!plain(a, 0) || !plain(b, 1) || ops[a].col != ops[b].col) return false;
    const int col = ops[a].col;
    const ColKind ka = t0.cols[col]->kind, kb = t1.cols[col]->kind;
    if (ka != kb || (ka != COL_STR && ka != COL_NUM)) return false;
    SimpleCol s{};
    s.k = k;
    s.kind = ka == COL_STR ? SK_STR : SK_NUM;
    s.col = col;
    s.null_level = wl[w0];
    s.else_level = prog.else_level;
    s.n_tests = prog.n_when - 1;
    s.stride = stride[k];
    for (int i = 0; i < s.n_tests; ++i) {
        const int w = w0 + 1 + i;
        if (wn[w] != 1) return false;
        const spk_instr &in = instr[wf[w]];
        if (in.a != a || in.b != b) return false;
        const bool str_op = (in.op == SPK_OP_STR_CMP && (in.cmp == SPK_CMP_EQ || in.cmp == SPK_CMP_NE)) ||
                            in.op == SPK_OP_JW || in.op == SPK_OP_LEV || in.op == SPK_OP_LEVRATIO;
        const bool num_op = in.op == SPK_OP_NUM_CMP || in.op == SPK_OP_ABSDIFF || in.op == SPK_OP_PERCDIFF;
        if (!(s.kind == SK_STR ? str_op : num_op)) return false;
        s.op[i] = in.op;
        s.cmp[i] = in.cmp;
        s.level[i] = wl[w];
        s.t[i] = in.t;
    }
    *out = s;
    return true;
}

spk_ctx::~spk_ctx() {
    for (spk::RawCol *r : raw) delete r;
    delete gcols;
    for (Slot &s : slot) delete s.gplan;
}

// A window's info block to the host, behind what `stream` holds so far.
static int read_info(spk_ctx *ctx, Slot &S, hipStream_t stream) {
    SPK_HIP(hipMemcpyAsync(S.h_info.p, S.xinfo.p, (size_t)ctx->gcols->n_all * 8, hipMemcpyDeviceToHost, stream));
    SPK_HIP(hipEventRecord(S.ev_info, stream));
    return SPK_OK;
}

namespace spk {
// Completes the last spk_gammas once its info blocks are on the host: a work-list overflow re-runs the
// exact phase with room for every listed cell, and cells with a string past SLOW_LIMIT units go through
// the huge pass.  *fixed = true when codes changed after the call returned (a consumer that already
// read them must read them again).  Called at the consumers' own synchronisation points.
static int settle_info(spk_ctx *ctx, bool *fixed);

int settle_gammas(spk_ctx *ctx, bool *fixed) {
    bool f = false;
    ctx->slot[0].stream = ctx->stream;  // a settlement's launches go where the context's work goes now
    SPK_TRY(settle_info(ctx, &f));
    if (fixed) *fixed = f;
    if (f) ++ctx->codes_fix_seq;  // a selection taken from the uncorrected codes is stale (spk_select_copy)
    // an asynchronous EM iteration enqueued on these codes read them before the correction: repeat it
    if (f && ctx->em_pending && ctx->em_seq == ctx->gamma_seq) {
        SPK_REQUIRE(ctx->em_kind == 0, SPK_E_STATE, "codes corrected under a pending finalize (settle before the histogram)");
        SPK_TRY(em_requeue(ctx));
    }
    return SPK_OK;
}

static int settle_slot(spk_ctx *ctx, Slot &S, bool *fixed);
// Every slot the last call used, then the call's figures: the windows' counts added to those of the windows
// settled before (exact_carry), their slow-list flags or-ed.
static int settle_info(spk_ctx *ctx, bool *fixed) {
    if (fixed) *fixed = false;
    bool pending = false, f = false;
    for (int i = 0; i < ctx->last_slots; ++i) pending = pending || ctx->slot[i].gamma_pending;
    if (!pending) return SPK_OK;
    for (int i = 0; i < ctx->last_slots; ++i) SPK_TRY(settle_slot(ctx, ctx->slot[i], &f));
    if (fixed) *fixed = f;
    if (!ctx->codes_valid || !ctx->gcols) return SPK_OK;  // the codes were replaced or invalidated since
    const int K = ctx->gcols->K;
    const bool carry = (int)ctx->exact_carry.size() == K;  // earlier windows of the same call
    ctx->last_exact.assign((size_t)K, 0);
    if (carry) ctx->last_exact = ctx->exact_carry;
    ctx->last_deferred = ctx->deferred_carry;
    ctx->slow_seen.assign((size_t)K, 0);
    for (int i = 0; i < ctx->last_slots; ++i) {
        const GammaPlan &G = *ctx->slot[i].gplan;
        for (int k = 0; k < K; ++k) {
            ctx->last_exact[k] += G.exact[k];
            ctx->slow_seen[k] |= G.slow_seen[k];
        }
        ctx->last_deferred += G.deferred;
    }
    ctx->slow_seen_valid = true;
    return SPK_OK;
}

// One window: *fixed is set when its codes changed (and left alone otherwise).
static int settle_slot(spk_ctx *ctx, Slot &S, bool *fixed) {
    if (!S.gamma_pending) return SPK_OK;
    // the info block is on the host once the readback behind it completed (later work -- an EM
    // iteration enqueued meanwhile -- keeps running)
    SPK_HIP(hipEventSynchronize(S.ev_info));
    S.gamma_pending = false;
    if (!ctx->codes_valid || !ctx->gcols || !S.gplan) return SPK_OK;  // the codes were replaced or invalidated since
    const GammaCols &C = *ctx->gcols;
    GammaPlan &G = *S.gplan;
    const int K = C.K;
    if (S.h_info.p[2 * K]) {
        // the exact lists did not fit: nothing of the phase ran; grow them and run the phase again
        const int64_t cap = S.h_info.p[2 * K + 1];
        SPK_HIP(hipMemsetAsync(S.xinfo.p + C.n_info, 0, (size_t)(C.n_cnt + 2) * 8, S.stream));
        SPK_TRY(enqueue_phase(ctx, S, cap));
        SPK_TRY(read_info(ctx, S, S.stream));
        SPK_HIP(hipStreamSynchronize(S.stream));
        *fixed = true;
        if (S.h_info.p[2 * K]) {
            ctx->codes_valid = false;
            SPK_REQUIRE(false, SPK_E_STATE, "spk_gammas: exact work list sizing failed");
        }
    }
    const unsigned int *h_slow = reinterpret_cast<const unsigned int *>(S.h_info.p + C.n_info);
    {  // slow-list kernels this call left out although the exact pass did list cells: run them now
        bool ran = false;
        ColSet jk{};
        for (int k = 0; k < K; ++k) {
            if (k >= (int)G.slow_skipped.size() || !G.slow_skipped[k] || !h_slow[k]) continue;
            const int si = C.simple_of[k];
            const bool lev = si >= 0 && C.simple[si].cls == SC_LEV;
            if (!lev && jk.n < 4) jk.k[jk.n++] = k;
            else SPK_TRY(enqueue_slow(ctx, S, k, nullptr));
            ran = true;
        }
        if (jk.n) SPK_TRY(enqueue_slow(ctx, S, -1, &jk));
        if (ran) {
            SPK_TRY(read_info(ctx, S, S.stream));
            SPK_HIP(hipStreamSynchronize(S.stream));
            *fixed = true;
        }
        G.slow_skipped.assign((size_t)K, 0);
    }
    int err = 0;
    std::memcpy(&err, S.h_info.p + C.n_info + C.n_cnt, sizeof(err));
    if (err & 2) {
        ctx->codes_valid = false;
        SPK_REQUIRE(false, SPK_E_INVALID, "spk_gammas: unknown instruction");
    }
    int64_t n_huge = 0;
    G.deferred = 0;
    for (int k = 0; k < K; ++k) {
        G.exact[k] = S.h_info.p[K + k];
        G.slow_seen[k] = h_slow[k] ? 1 : 0;
        G.deferred += h_slow[k];
        n_huge += h_slow[2 * K + k];
    }
    G.xbase.assign(S.h_info.p, S.h_info.p + K);
    if (n_huge) {
        SPK_TRY(run_huge(ctx, S, h_slow + 2 * K));
        *fixed = true;
    }
    return SPK_OK;
}
}  // namespace spk

// ---- spk_gammas, stage by stage ------------------------------------------------------------------------------
// The arguments of spk_gammas.
struct Program {
    int n_cols;
    const spk_column_program *cols;
    int n_when;
    const int32_t *when_first_instr, *when_n_instr, *when_level;
    int n_instr;
    const spk_instr *instr;
    int n_operands;
    const spk_operand *operands;
    int n_lits;
    const int64_t *lit_offsets;
    const uint8_t *lit_utf8;
};

// Stage 1: host-side validation of the program against the loaded tables; nlev = the columns' level counts.
static int validate_program(const Program &p, const Table &t0, const Table &t1, std::vector<int32_t> *nlev) {
    for (int i = 0; i < p.n_operands; ++i) {
        const spk_operand &o = p.operands[i];
        if (o.kind == 0) {
            const Table &t = o.side ? t1 : t0;
            SPK_REQUIRE(o.col >= 0 && o.col < (int)t.cols.size() && t.cols[o.col] && t.cols[o.col]->kind != COL_NONE,
                        SPK_E_INVALID, "spk_gammas: operand references a column that was not loaded");
        }
        if (o.kind == 1 || (o.kind == 0 && o.lit >= 0))
            SPK_REQUIRE(o.lit < p.n_lits, SPK_E_INVALID, "spk_gammas: literal index out of range");
    }
    nlev->resize((size_t)p.n_cols);
    for (int k = 0; k < p.n_cols; ++k) {
        const spk_column_program &c = p.cols[k];
        (*nlev)[k] = c.n_levels;
        SPK_REQUIRE(c.first_when >= 0 && c.first_when + c.n_when <= p.n_when, SPK_E_INVALID, "spk_gammas: when range");
        SPK_REQUIRE(c.else_level >= -1 && c.else_level < c.n_levels, SPK_E_INVALID,
                    "spk_gammas: else level out of range");
        for (int w = c.first_when; w < c.first_when + c.n_when; ++w) {
            SPK_REQUIRE(p.when_level[w] >= -1 && p.when_level[w] < c.n_levels, SPK_E_INVALID,
                        "spk_gammas: THEN level out of range");
            SPK_REQUIRE(p.when_first_instr[w] >= 0 && p.when_n_instr[w] >= 1 && p.when_n_instr[w] <= 16 &&
                            p.when_first_instr[w] + p.when_n_instr[w] <= p.n_instr,
                        SPK_E_INVALID, "spk_gammas: predicate range (max 16 RPN instructions)");
        }
    }
    for (int i = 0; i < p.n_instr; ++i) {
        const spk_instr &in = p.instr[i];
        bool logical = in.op == SPK_OP_AND || in.op == SPK_OP_OR || in.op == SPK_OP_NOT || in.op == SPK_OP_CONST;
        if (!logical) {
            SPK_REQUIRE(in.a >= 0 && in.a < p.n_operands, SPK_E_INVALID, "spk_gammas: operand index");
            bool two = !(in.op == SPK_OP_ISNULL || in.op == SPK_OP_NOTNULL || in.op == SPK_OP_LEN);
            if (two) SPK_REQUIRE(in.b >= 0 && in.b < p.n_operands, SPK_E_INVALID, "spk_gammas: operand index");
        }
        if (in.op == SPK_OP_CONST) SPK_REQUIRE(in.i0 >= 0 && in.i0 <= 2, SPK_E_INVALID, "spk_gammas: constant");
    }
    return SPK_OK;
}

// Stage 2: the literals as UTF-16, one buffer, with an empty literal at the end.
struct Literals {
    std::vector<uint16_t> units;
    std::vector<int64_t> off;
    std::vector<int32_t> len, cplen;
};
static Literals literals_utf16(const Program &p) {
    Literals l;
    for (int i = 0; i < p.n_lits; ++i) {
        int32_t ncp = 0;
        auto u = utf8_to_utf16(p.lit_utf8 + p.lit_offsets[i], p.lit_offsets[i + 1] - p.lit_offsets[i], &ncp);
        l.off.push_back((int64_t)l.units.size());
        l.len.push_back((int32_t)u.size());
        l.cplen.push_back(ncp);
        l.units.insert(l.units.end(), u.begin(), u.end());
    }
    l.units.resize(l.units.size() + 8, 0);  // 4-unit vector reads past a literal's end stay in the buffer
    l.off.push_back((int64_t)l.units.size());
    l.len.push_back(0);
    l.cplen.push_back(0);
    return l;
}

// Stage 3: which columns the template filter takes (`C.simple`, laid out in the row image) and which the
// interpreter (`complex_k`), with everything the passes decide per column.
struct ColumnPlan {
    GammaCols C;
    std::vector<int32_t> complex_k;
    std::vector<int16_t> thr_tab;  // threshold tables of the Levenshtein-ratio tests (SimpleCol.thr_off)
    int64_t img_stride = 0;
    bool long_exact = false;       // a free-text Levenshtein column: its exact and slow passes dominate the pass
};

// Sketch rows of the template Levenshtein columns' strings that `wanted` names, built on first use.
template <class Wanted, class Build>
static int build_sketch_rows(spk_ctx *ctx, Table &t0, Table &t1, std::vector<SimpleCol> &simple, Wanted wanted,
                             DevBuf<uint4> Column::*rows, Build build) {
    bool built[2] = {false, false};
    for (SimpleCol &sc : simple) {
        if (!wanted(sc)) continue;
        for (int s = 0; s < 2; ++s) {
            Table &t = s ? t1 : t0;
            Column *c = t.cols[sc.col];
            if (c->kind != COL_STR || (c->*rows).n || t.n <= 0) continue;
            SPK_TRY(build(ctx, t.n, c));
            t.desc_dirty = true;
            built[s] = true;
        }
    }
    if (built[0]) SPK_TRY(ensure_desc(ctx, t0));
    if (built[1]) SPK_TRY(ensure_desc(ctx, t1));
    return SPK_OK;
}

static int plan_columns(spk_ctx *ctx, const Program &p, const Literals &lits, Table &t0, Table &t1, ColumnPlan *out) {
    SPK_TRY(ensure_desc(ctx, t0));
    SPK_TRY(ensure_desc(ctx, t1));
    const int K = p.n_cols;
    GammaCols &C = out->C;
    std::vector<SimpleCol> &simple = C.simple;
    std::vector<int32_t> &complex_k = out->complex_k;
    for (int k = 0; k < K; ++k) {
        SimpleCol sc;
        if (ctx->filter_mode != 0 &&
            classify_simple(k, p.cols[k], p.when_first_instr, p.when_n_instr, p.when_level, p.instr, p.operands, t0, t1,
                            ctx->stride, &sc))
            simple.push_back(sc);
        else
            complex_k.push_back(k);
    }
    auto free_text = [&](const SimpleCol &sc) {  // rows past 64 UTF-8 bytes on both sides (planes_hi)
        const Column *a = t0.cols[sc.col], *b = t1.cols[sc.col];
        return sc.kind == SK_STR && a && b && a->planes_hi.n && b->planes_hi.n;
    };
    for (SimpleCol &sc : simple) {
        sc.cls = simple_class(sc);
        prepare_tests(sc);
        sc.np = N_PLANES;
        if (sc.kind == SK_STR && t0.cols[sc.col]->unit_bits && t1.cols[sc.col]->unit_bits) {
            const uint32_t any = t0.cols[sc.col]->unit_or | t1.cols[sc.col]->unit_or;
            const uint32_t all = t0.cols[sc.col]->unit_and & t1.cols[sc.col]->unit_and;
            while (sc.np > 5 && (((any ^ all) >> (sc.np - 1)) & 1u) == 0) --sc.np;  // top bit constant
        }
        sc.has_ids = (t0.cols[sc.col]->has_ids && t1.cols[sc.col]->has_ids) ? 1 : 0;
        implied_equal(ctx, t0, t1, sc);
    }
    // character-bag rows of the free-text Levenshtein columns' strings (k_compact_lev).
    // Free-text only: in cfg2's emails the bound decided 15 % of the listed cells (1.23 of 8.10 M), and the
    // compaction's gathers cost more than the scans it saved (γ pass 1.070 -> 1.168 ms; cfg5's addresses
    // 4.88 -> 3.85 ms; profiles/r5_ab_lev_bag.log).
    if (ctx->lev_bag)
        SPK_TRY(build_sketch_rows(
            ctx, t0, t1, simple, [&](const SimpleCol &sc) { return sc.cls == SC_LEV && free_text(sc); }, &Column::bag,
            build_bag_rows));
    // positional sketch rows of the other template Levenshtein columns' strings (the filter's two-segment bound)
    for (SimpleCol &sc : simple)
        sc.pos = (sc.cls == SC_LEV && sc.kind == SK_STR && ctx->lev_bound == 1 && !free_text(sc)) ? 1 : 0;
    SPK_TRY(build_sketch_rows(
        ctx, t0, t1, simple, [](const SimpleCol &sc) { return sc.pos != 0; }, &Column::pos, build_pos_rows));
    for (SimpleCol &sc : simple) {
        for (int i = 0; i < MAX_TESTS; ++i) sc.thr_off[i] = -1;
        if (sc.cls != SC_LEV) continue;
        for (int i = 0; i < sc.n_tests; ++i) {
            if (sc.op[i] != SPK_OP_LEVRATIO || (sc.cmp[i] != SPK_CMP_LE && sc.cmp[i] != SPK_CMP_LT)) continue;
            sc.thr_off[i] = (int32_t)out->thr_tab.size();
            for (int S = 0; S < THR_S; ++S) {
                // `v / den cmp t` holds for v <= the entry (monotone in v); S = 0 is NULL (den = 0)
                int th = -1;
                const double den = (double)S / 2.0;
                for (int v = 0; v < THR_S && S > 0; ++v)
                    if (host_cmp((double)v / den, sc.t[i], sc.cmp[i])) th = v;
                    else break;
                out->thr_tab.push_back((int16_t)th);
            }
        }
    }
    out->img_stride = layout_image(simple);
    // simple columns the filter kernel cannot take (no filter class, no room in the image) join the
    // interpreter's columns
    for (size_t i = 0; i < simple.size();) {
        if (simple[i].cls == SC_NONE) {
            complex_k.push_back(simple[i].k);
            simple.erase(simple.begin() + (long)i);
        } else {
            ++i;
        }
    }
    std::sort(complex_k.begin(), complex_k.end());

    // the decisions of the exact and slow passes (host decisions only; the lists are sized on the device by k_prefix)
    C.K = K;
    C.simple_of.assign(K, -1);
    for (size_t i = 0; i < simple.size(); ++i) C.simple_of[simple[i].k] = (int)i;
    C.may_exact.assign(K, 1);  // columns whose filter can leave cells undecided (a dictionary-id equality or
                               // numeric column never does)
    for (const SimpleCol &sc : simple)
        if (sc.kind == SK_NUM || sc.cls == SC_NUM || (sc.cls == SC_EQ && sc.has_ids)) C.may_exact[sc.k] = 0;
    C.free_text.assign(K, 0);
    C.bag.assign(K, 0);  // free-text Levenshtein columns with character-bag rows (k_compact_lev)
    for (const SimpleCol &sc : simple) {
        const Column *a = t0.cols[sc.col], *b = t1.cols[sc.col];
        C.free_text[sc.k] = (a && b && a->planes_hi.n && b->planes_hi.n) ? 1 : 0;
        C.bag[sc.k] = (C.free_text[sc.k] && sc.cls == SC_LEV && a->bag.n && b->bag.n && ctx->lev_bag) ? 1 : 0;
        out->long_exact = out->long_exact || (sc.cls == SC_LEV && C.free_text[sc.k]);
    }
    C.setsim.assign(K, 0);
    for (int k = 0; k < K; ++k)
        for (int w = p.cols[k].first_when; w < p.cols[k].first_when + p.cols[k].n_when; ++w)
            for (int i = p.when_first_instr[w]; i < p.when_first_instr[w] + p.when_n_instr[w]; ++i)
                if (p.instr[i].op == SPK_OP_JACCARD || p.instr[i].op == SPK_OP_COSINE) C.setsim[k] = 1;
    C.huge_in_slow.assign(K, 0);  // column k's huge list: slow-list region (Levenshtein) or exact-list region
    for (int k = 0; k < K; ++k)
        C.huge_in_slow[k] = (C.may_exact[k] && C.simple_of[k] >= 0 && simple[C.simple_of[k]].cls == SC_LEV) ? 1 : 0;
    // One device info block per window, read back with one copy: xinfo (k_prefix: list bases and counts,
    // overflow, total), then the slow / rest / huge list lengths (3K uint32) and the error word, both zeroed per
    // window.
    C.n_info = 2 * K + 2;
    C.n_cnt = (3 * K + 1) / 2;          // int64 slots of the 3K uint32 list lengths
    C.n_all = C.n_info + C.n_cnt + 2;   // + the error word and k_prefix's completion counter
    // every string a program can meet is a row of a loaded string column (UTF-8 bytes bound its UTF-16
    // units), a substring of one, or a literal: the huge pass's scratch per lane
    C.max_units = 1;
    for (const Table *t : {&t0, &t1})
        for (const Column *c : t->cols)
            if (c && c->kind == COL_STR) C.max_units = std::max<int64_t>(C.max_units, c->max_bytes);
    for (int i = 0; i < p.n_lits; ++i) C.max_units = std::max<int64_t>(C.max_units, lits.len[i]);
    return SPK_OK;
}

// Stage 4: every program array goes up in one packed copy into a buffer the context keeps (ctx->last_blob is
// its host copy).  The device keeps the last blob: an unchanged program (every call of an EM run) is not re-sent.
struct BlobOffsets {
    size_t prog, wf, wn, wl, instr, ops, lu, loff, llen, lcp, stride, simple, complex_k, thr;
};
static int upload_program(spk_ctx *ctx, const Program &p, const Literals &lits, const ColumnPlan &cp, BlobOffsets *o,
                          bool *fresh_blob) {
    std::vector<uint8_t> blob;
    auto put = [&](const auto *src, size_t n) -> size_t {
        const size_t off = (blob.size() + 15) & ~(size_t)15;
        blob.resize(off + (n ? n : 1) * sizeof(*src), 0);
        if (n) std::memcpy(blob.data() + off, src, n * sizeof(*src));
        return off;
    };
    o->prog = put(p.cols, (size_t)p.n_cols);
    o->wf = put(p.when_first_instr, (size_t)p.n_when);
    o->wn = put(p.when_n_instr, (size_t)p.n_when);
    o->wl = put(p.when_level, (size_t)p.n_when);
    o->instr = put(p.instr, (size_t)p.n_instr);
    o->ops = put(p.operands, (size_t)p.n_operands);
    o->lu = put(lits.units.data(), lits.units.size());
    o->loff = put(lits.off.data(), lits.off.size());
    o->llen = put(lits.len.data(), lits.len.size());
    o->lcp = put(lits.cplen.data(), lits.cplen.size());
    o->stride = put(ctx->stride.data(), ctx->stride.size());
    o->simple = put(cp.C.simple.data(), cp.C.simple.size());
    o->complex_k = put(cp.complex_k.data(), cp.complex_k.size());
    o->thr = put(cp.thr_tab.data(), cp.thr_tab.size());
    *fresh_blob = ctx->prog_blob.p && ctx->prog_blob.n >= blob.size() && ctx->last_blob == blob;
    if (!*fresh_blob || ctx->slow_key_pairs != ctx->pairs_epoch || ctx->slow_key_tables != ctx->table_epoch)
        ctx->slow_seen_valid = false;
    ctx->slow_key_pairs = ctx->pairs_epoch;
    ctx->slow_key_tables = ctx->table_epoch;
    if (!*fresh_blob) {
        SPK_TRY(ctx->prog_blob.alloc(blob.size()));
        SPK_HIP(hipMemcpyAsync(ctx->prog_blob.p, blob.data(), blob.size(), hipMemcpyHostToDevice, ctx->stream));
        ctx->last_blob = std::move(blob);
    }
    return SPK_OK;
}

// Stage 5: the windows.  Ordinal windows: the filter's work lists and the exact / slow passes hold
// window-relative pair ordinals as int32 (and the filter walks them in uint32), so a pair set of more than
// ~2^31 pairs runs as consecutive windows of equal size.  Every window but the last is settled (list overflow,
// skipped slow lists, huge cells) before the next one reuses the lists; the last is left pending as usual.
// The two-stream split (spk_ctx::slot): two windows at once, one per stream.
struct WindowLayout {
    int64_t P = 0, W = 0, n_win = 1;  // pairs, pairs per window (window 0 is the largest), windows
    bool split = false;
    int64_t max_regions = 0;
    int n_regions_max = 0;            // regions of window 0
    // one filter workgroup per region of consecutive pair ordinals (a multiple of the wave size)
    int regions_of(int64_t pw) const {
        return (int)std::max<int64_t>(1, std::min<int64_t>(max_regions, (pw + F_THREADS - 1) / F_THREADS));
    }
};
static WindowLayout layout_windows(const spk_ctx *ctx, bool long_exact) {
    WindowLayout L;
    const int64_t P = L.P = ctx->n_pairs;
    const int64_t WMAX = ((int64_t)1 << 31) - ((int64_t)1 << 22);
    const int64_t wcap = ctx->gamma_window > 0 ? std::min<int64_t>(ctx->gamma_window, WMAX) : WMAX;
    const int64_t n_win0 = std::max<int64_t>(1, (P + wcap - 1) / wcap);
    L.split = ctx->gamma_streams >= 2 && ctx->gamma_window == 0 && n_win0 == 1 &&
              P >= std::max<int64_t>(ctx->split_min, 256);
    // Window 0 (the context stream, which starts first and continues after the join) takes 60 % of the pairs, or half
    // when a free-text Levenshtein column's long exact and slow passes dominate the pass: measured best shares, cfg2
    // 0.966 -> 0.943 ms per step at 60 %, cfg5 best at 50 % (profiles/r6_ab_split_share.log)
    L.W = L.split ? (P * (long_exact ? 500 : 600) / 1000 + 63) / 64 * 64
                  : (n_win0 == 1 ? P : ((P + n_win0 - 1) / n_win0 + 63) / 64 * 64);
    // rounding W up to a multiple of 64 can leave trailing windows empty (small test windows): count the
    // windows from W itself
    L.n_win = L.split ? 2 : (n_win0 == 1 ? 1 : (P + L.W - 1) / L.W);
    // 20 regions (256-thread workgroups) per CU: four rounds of the 5 resident workgroups a CU holds
    // at the filter's 96-VGPR cap, so the regions' uneven work evens out (measured best of 1280 ..
    // 20480 on MI355X: 5120 regions 1.76 ms vs 2048 regions 1.86 ms for the cfg2 pass)
    L.max_regions = 20 * (int64_t)ctx->n_cu;
    L.n_regions_max = L.regions_of(L.W);
    return L;
}

// Stage 6: the codes, and the buffers of every slot the call uses (slot 1's stream and events on the first split).
// Work lists only for the columns whose filter can leave cells undecided: one list of W pair indices each.  Every
// (column, region) count is written by the filter launch that covers the region, so region_count needs no memset.
static int alloc_slots(spk_ctx *ctx, const WindowLayout &L, const GammaCols &C, int n_slots) {
    if (L.split && !ctx->split_ready) {
        SPK_HIP(hipStreamCreateWithFlags(&ctx->slot[1].stream, hipStreamNonBlocking));
        SPK_HIP(hipEventCreateWithFlags(&ctx->slot[1].ev_info, hipEventDisableTiming));
        SPK_HIP(hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
        SPK_HIP(hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming));
        ctx->split_ready = true;
    }
    SPK_TRY(ctx->codes.alloc((size_t)(L.P + 1) * ctx->code_bytes));
    int n_lists = 0;
    for (int k = 0; k < C.K; ++k) n_lists += C.may_exact[k] ? 1 : 0;
    for (int i = 0; i < n_slots; ++i) {
        Slot &S = ctx->slot[i];
        SPK_TRY(S.work.alloc((size_t)std::max(n_lists, 1) * (size_t)L.W + 1));
        SPK_TRY(S.region_count.alloc((size_t)C.K * L.n_regions_max));
        SPK_TRY(S.xinfo.alloc((size_t)C.n_all));
        SPK_TRY(S.h_info.grow((size_t)C.n_all));
        SPK_TRY(S.xpref.alloc((size_t)C.K * (L.n_regions_max + 1)));
        if (!S.gplan) S.gplan = new GammaPlan();
    }
    return SPK_OK;
}

// Stage 7: the arguments every window shares (its own in run_window).
static GammaArgs gamma_args(const spk_ctx *ctx, const Table &t0, const Table &t1, const ColumnPlan &cp,
                            const BlobOffsets &o) {
    GammaArgs A{};
    uint8_t *base = ctx->prog_blob.p;
    auto at = [&](auto *&dst, size_t off) { dst = reinterpret_cast<std::remove_reference_t<decltype(dst)>>(base + off); };
    A.cols0 = t0.d_desc.p;
    A.cols1 = t1.d_desc.p;
    A.pl = ctx->pl.p;
    A.pr = ctx->pr.p;
    A.P = ctx->n_pairs;
    A.K = cp.C.K;
    at(A.progs, o.prog);
    at(A.when_first, o.wf);
    at(A.when_n, o.wn);
    at(A.when_level, o.wl);
    at(A.instr, o.instr);
    at(A.ops, o.ops);
    at(A.lit_units, o.lu);
    at(A.lit_off, o.loff);
    at(A.lit_len, o.llen);
    at(A.lit_cplen, o.lcp);
    at(A.stride, o.stride);
    at(A.simple, o.simple);
    at(A.complex_k, o.complex_k);
    at(A.thr, o.thr);
    A.n_thr = (int)cp.thr_tab.size();
    A.codes = ctx->codes.p;
    A.code16 = ctx->code_bytes == 2;
    for (int k = 0, n = 0; k < cp.C.K; ++k) A.wslot[k] = cp.C.may_exact[k] ? n++ : 0;
    A.n_simple = (int)cp.C.simple.size();
    A.n_complex = (int)cp.complex_k.size();
    return A;
}

// What the windows of one call run with.
struct GammaRun {
    const GammaArgs &A;
    const WindowLayout &L;
    const ViewLaunch *V;  // rule 1's view-ordered images, or null
};

// Stage 8: graph replay -- everything the launches' arguments and decisions depend on.
static std::vector<int64_t> graph_key(const spk_ctx *ctx, const GammaRun &R) {
    auto ptr = [](const void *q) { return (int64_t)(uintptr_t)q; };
    const WindowLayout &L = R.L;
    std::vector<int64_t> key = {
        L.P, L.n_win, L.split ? 1 : 0, L.W, R.A.K, ctx->code_bytes, (int64_t)ctx->pairs_epoch, (int64_t)ctx->table_epoch,
        (int64_t)std::hash<std::string>()(std::string(ctx->last_blob.begin(), ctx->last_blob.end())), ctx->lev_kernel,
        ctx->lev_bag ? 1 : 0, ctx->lev_bound, ctx->filter_mode, ctx->use_views, ctx->slow_force_skip ? 1 : 0,
        R.V ? 1 : 0, ptr(ctx->codes.p), ptr(ctx->pl.p), ptr(ctx->pr.p), ptr(ctx->pvl.p), ptr(ctx->prog_blob.p),
        ptr(ctx->img[0].p), ptr(ctx->img[1].p), ctx->slow_seen_valid ? 1 : 0, (int64_t)ctx->timing};
    for (const Slot &S : ctx->slot)
        key.insert(key.end(), {ptr(S.stream), ptr(S.work.p), ptr(S.xlist.p), ptr(S.xinfo.p), ptr(S.xpref.p),
                               ptr(S.region_count.p), S.xcap});
    for (uint8_t f : ctx->slow_seen) key.push_back(f);
    for (int v = 0; v < MAX_VIEWS; ++v) key.push_back(ptr(ctx->vimg[v][0].p));
    return key;
}

// Stage 9: window w, pairs [w W, min((w + 1) W, P)), enqueued on the slot's stream: filter, exact and slow passes.
static int run_window(spk_ctx *ctx, const GammaRun &R, Slot &S, int64_t w) {
    const GammaCols &C = *ctx->gcols;
    GammaPlan &G = *S.gplan;
    const int64_t b = w * R.L.W, Pw = std::min<int64_t>(R.L.W, R.L.P - b);
    const int n_regions = R.L.regions_of(Pw);
    const int64_t region_len = ((Pw + n_regions - 1) / n_regions + 63) / 64 * 64;
    GammaArgs &AW = G.A = R.A;  // the window [b, b + Pw) as a pair set of its own
    AW.err = reinterpret_cast<int *>(S.xinfo.p + C.n_info + C.n_cnt);
    AW.work = S.work.p;
    AW.region_count = S.region_count.p;
    AW.slow_count = reinterpret_cast<unsigned int *>(S.xinfo.p + C.n_info);
    AW.pl = ctx->pl.p + b;
    AW.pr = ctx->pr.p + b;
    AW.P = Pw;
    AW.codes = ctx->codes.p + b * ctx->code_bytes;
    AW.region_len = region_len;
    AW.n_regions = n_regions;
    std::vector<SimpleCol> sw = C.simple;  // implied ranges relative to the window
    for (SimpleCol &sc : sw) {
        sc.imp_lo = std::min<int64_t>(std::max<int64_t>(sc.imp_lo - b, 0), Pw);
        sc.imp_hi = std::min<int64_t>(std::max<int64_t>(sc.imp_hi - b, 0), Pw);
        if (sc.imp_hi <= sc.imp_lo) sc.imp_lo = sc.imp_hi = 0;
    }
    G.first = b;
    G.n_regions = n_regions;
    G.g_exact = std::max<int64_t>(1, std::min<int64_t>(8 * (int64_t)ctx->n_cu, (Pw + X_THREADS - 1) / X_THREADS));
    G.xbase.assign((size_t)C.K, 0);
    G.exact.assign((size_t)C.K, 0);
    G.slow_seen.assign((size_t)C.K, 0);
    G.deferred = 0;
    SPK_HIP(hipMemsetAsync(S.xinfo.p + C.n_info, 0, (size_t)(C.n_cnt + 2) * 8, S.stream));
    int64_t va = n_regions, vb = n_regions;  // regions over rule 1's view-ordered image: [va, vb)
    if (Pw > 0) {
        if (R.V) {  // regions [i L, min((i + 1) L, Pw)) inside the window's part of [V.lo, V.hi)
            const int64_t lo = std::min<int64_t>(std::max<int64_t>(R.V->lo - b, 0), Pw);
            const int64_t hi = std::min<int64_t>(std::max<int64_t>(R.V->hi - b, 0), Pw);
            va = std::min<int64_t>(n_regions, (lo + region_len - 1) / region_len);
            vb = hi >= Pw ? n_regions : std::min<int64_t>(n_regions, hi / region_len);
            vb = hi > lo ? std::max<int64_t>(va, vb) : va;
        }
        ctx->last_view_regions += vb - va;
        // the filter pass (the interpreter's columns add to the codes the template filter sets)
        if (sw.empty()) SPK_HIP(hipMemsetAsync(AW.codes, 0, (size_t)Pw * ctx->code_bytes, S.stream));
        if (!sw.empty()) {
            SPK_TRY(launch_template_filter(S.stream, AW, sw, 0, va));
            if (vb > va) {
                GammaArgs VA = AW;
                VA.pl = ctx->pvl.p - ctx->pv_base + b;  // pl[p] = view position of pair b + p (>= pv_base)
                VA.pr = ctx->pvr.p - ctx->pv_base + b;
                VA.img0 = R.V->img0;
                VA.img1 = R.V->img1;
                SPK_TRY(launch_template_filter(S.stream, VA, sw, va, vb));
            }
            SPK_TRY(launch_template_filter(S.stream, AW, sw, vb, n_regions));
        }
        if (AW.n_complex) {
            k_gamma_filter<<<(unsigned)n_regions, F_THREADS, 0, S.stream>>>(AW);
            SPK_HIP(hipGetLastError());
        }
    }
    const int64_t cap = std::max<int64_t>(S.xcap, std::max<int64_t>(Pw, 1 << 16));
    return enqueue_phase(ctx, S, cap, /*skip=*/true);
}

// Once slot 1's stream has forked from the context stream, every way out joins it back: without the join a later
// call could rewrite the codes while window 1's kernels of a failed call still run.
struct SplitJoin {
    spk_ctx *ctx;
    bool recorded = false, waited = false;
    int record() {  // what slot 1's stream holds so far ...
        recorded = true;
        SPK_HIP(hipEventRecord(ctx->ev_join, ctx->slot[1].stream));
        return SPK_OK;
    }
    int wait() {  // ... is what the context stream waits for
        waited = true;
        SPK_HIP(hipStreamWaitEvent(ctx->slot[0].stream, ctx->ev_join, 0));
        return SPK_OK;
    }
    ~SplitJoin() {
        if (!recorded) (void)record();
        if (!waited) (void)wait();
    }
};

// The exact lists of the window just settled in S, behind those of the call's earlier windows (ctx->list_carry):
// the next window overwrites the slot's lists, and spk_gammas_exact_list reports the whole call's.  Device-to-device
// copies on the slot's stream, ahead of the next window's launches.
static int carry_lists(spk_ctx *ctx, Slot &S) {
    const GammaPlan &G = *S.gplan;
    int64_t need = ctx->xcarry_used;
    for (int64_t n : G.exact) need += n;
    if (need > (int64_t)ctx->xcarry.n) {
        DevBuf<int32_t> grown;
        SPK_TRY(grown.alloc((size_t)std::max<int64_t>(need, 2 * (int64_t)ctx->xcarry.n)));
        if (ctx->xcarry_used) {
            SPK_HIP(hipMemcpyAsync(grown.p, ctx->xcarry.p, (size_t)ctx->xcarry_used * 4, hipMemcpyDeviceToDevice, S.stream));
            SPK_HIP(hipStreamSynchronize(S.stream));  // before the old buffer is freed
        }
        ctx->xcarry = std::move(grown);
    }
    for (int k = 0; k < (int)G.exact.size(); ++k) {
        if (G.exact[k] <= 0) continue;
        SPK_HIP(hipMemcpyAsync(ctx->xcarry.p + ctx->xcarry_used, S.xlist.p + G.xbase[k], (size_t)G.exact[k] * 4,
                               hipMemcpyDeviceToDevice, S.stream));
        ctx->list_carry.push_back({k, G.first, ctx->xcarry_used, G.exact[k]});
        ctx->xcarry_used += G.exact[k];
    }
    return SPK_OK;
}

// Stage 10a: the call's windows.  in_graph: under stream capture, which takes no readback (the caller reads the
// info blocks behind the graph).
static int run_windows(spk_ctx *ctx, const GammaRun &R, bool in_graph) {
    ctx->last_view_regions = 0;
    ctx->list_carry.clear();
    ctx->xcarry_used = 0;
    if (R.L.split) {
        // window 1's stream starts after everything queued so far (images, program blob, earlier reads of the
        // codes), together with window 0.  Starting it after window 0's filter instead (so that its filter runs
        // beside window 0's exact passes) measured slower: the short JW launch then waited behind the second
        // filter's workgroups (cfg2 0.99 -> 1.02 ms per step, profiles/r6_ab_gamma_streams.log).
        SPK_HIP(hipEventRecord(ctx->ev_fork, ctx->slot[0].stream));
        SPK_HIP(hipStreamWaitEvent(ctx->slot[1].stream, ctx->ev_fork, 0));
        SplitJoin fork{ctx};
        // each window's info block on its own stream (window 0's not behind the join); the join is recorded right
        // after window 1's last kernel, so the context stream waits for nothing else of it, and waited for after the
        // readback is enqueued
        SPK_TRY(run_window(ctx, R, ctx->slot[0], 0));
        if (!in_graph) SPK_TRY(read_info(ctx, ctx->slot[0], ctx->slot[0].stream));
        SPK_TRY(run_window(ctx, R, ctx->slot[1], 1));
        SPK_TRY(fork.record());
        if (!in_graph) SPK_TRY(read_info(ctx, ctx->slot[1], ctx->slot[1].stream));
        return fork.wait();
    }
    Slot &S = ctx->slot[0];
    for (int64_t w = 0; w < R.L.n_win; ++w) {
        SPK_TRY(run_window(ctx, R, S, w));
        if (w + 1 == R.L.n_win) break;
        // settle this window before the next one reuses the lists
        SPK_TRY(read_info(ctx, S, S.stream));
        S.gamma_pending = true;
        ctx->codes_valid = true;
        const int rc = settle_info(ctx, nullptr);
        ctx->codes_valid = false;  // (the call is not through)
        SPK_TRY(rc);
        ctx->exact_carry = ctx->last_exact;
        ctx->deferred_carry = ctx->last_deferred;
        SPK_TRY(carry_lists(ctx, S));
    }
    return SPK_OK;
}

// Stage 10b: the windows enqueued directly, captured into a graph (the second call with a key) or replayed from it
// (later calls with that key).  *via_graph: the pass ran as a graph launch.
static int run_pass(spk_ctx *ctx, const GammaRun &R, bool fresh_blob, bool *via_graph) {
    *via_graph = false;
    const int n_slots = R.L.split ? 2 : 1;
    const std::vector<int64_t> gkey = graph_key(ctx, R);
    const bool graphable = ctx->use_graph && !ctx->timing_exact && R.L.P > 0 && fresh_blob && (R.L.split || R.L.n_win == 1);
    const bool replay = graphable && ctx->gexec && gkey == ctx->gkey;
    bool cap = graphable && !replay && gkey == ctx->gkey_prev;  // the second call with this key
    ctx->gkey_prev = gkey;
    *via_graph = replay;
    if (replay) {
        // the slots' plans as the captured call left them; the slow-list launches it skipped
        for (int i = 0; i < n_slots; ++i) ctx->slot[i].gplan->slow_skipped = ctx->gskip[i];
        ctx->last_view_regions = ctx->gview_regions;
        SPK_HIP(hipGraphLaunch(ctx->gexec, ctx->stream));
        ++ctx->graph_launches;
        return SPK_OK;
    }
    if (cap) {
        if (ctx->gexec) (void)hipGraphExecDestroy(ctx->gexec);
        if (ctx->graph) (void)hipGraphDestroy(ctx->graph);
        ctx->gexec = nullptr;
        ctx->graph = nullptr;
        ctx->gkey.clear();
        if (hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
            (void)hipGetLastError();
            cap = false;
            ctx->use_graph = false;
        }
    }
    int rc = run_windows(ctx, R, cap);
    if (cap) {
        hipGraph_t g = nullptr;
        hipError_t e = hipStreamEndCapture(ctx->stream, &g);
        if (rc == SPK_OK && e == hipSuccess) e = hipGraphInstantiate(&ctx->gexec, g, nullptr, nullptr, 0);
        if (rc == SPK_OK && e == hipSuccess) {
            ctx->graph = g;
            ctx->gkey = gkey;
            for (int i = 0; i < n_slots; ++i) ctx->gskip[i] = ctx->slot[i].gplan->slow_skipped;
            ctx->gview_regions = ctx->last_view_regions;
            rc = hipGraphLaunch(ctx->gexec, ctx->stream) == hipSuccess ? SPK_OK : SPK_E_HIP;
        } else {
            // nothing of the captured pass ran: no graphs on this context from now on, the pass enqueued directly
            if (g) (void)hipGraphDestroy(g);
            ctx->gexec = nullptr;
            (void)hipGetLastError();
            ctx->use_graph = false;
            cap = false;
            if (rc == SPK_OK) rc = run_windows(ctx, R, false);
        }
    }
    *via_graph = cap;
    return rc;
}

extern "C" int spk_gammas(spk_ctx *ctx, int n_cols, const spk_column_program *cols, int n_when,
                          const int32_t *when_first_instr, const int32_t *when_n_instr, const int32_t *when_level,
                          int n_instr, const spk_instr *instr, int n_operands, const spk_operand *operands, int n_lits,
                          const int64_t *lit_offsets, const uint8_t *lit_utf8) {
    SPK_REQUIRE(ctx && cols && n_cols >= 1, SPK_E_INVALID, "spk_gammas: bad args");
    SPK_REQUIRE(ctx->pairs_valid, SPK_E_STATE, "spk_gammas: no pairs");
    SPK_REQUIRE(n_operands < 4096 && n_instr >= 0 && n_when >= 0, SPK_E_LIMIT, "spk_gammas: program too large");
    SPK_HIP(hipSetDevice(ctx->device));
    ctx->slot[0].stream = ctx->stream;  // (spk_ctx_set_stream may have changed it since the last call)
#ifdef SPK_HOST_TIMING
    const auto ht0 = std::chrono::steady_clock::now();
#endif
    SPK_TRY(settle_gammas(ctx, nullptr));  // the previous call's capacity feedback (its codes are replaced)
#ifdef SPK_HOST_TIMING
    const auto ht1 = std::chrono::steady_clock::now();
#endif
    const Program prog{n_cols, cols, n_when, when_first_instr, when_n_instr, when_level, n_instr, instr, n_operands,
                       operands, n_lits, lit_offsets, lit_utf8};
    Table &t0 = ctx->table[0];
    Table &t1 = ctx->side_table(1);
    std::vector<int32_t> nlev;
    SPK_TRY(validate_program(prog, t0, t1, &nlev));
    ctx->codes_valid = false;  // codes are rewritten in place below
    SPK_TRY(set_pattern_space(ctx, n_cols, nlev.data()));
    const Literals lits = literals_utf16(prog);
    ColumnPlan cp;
    SPK_TRY(plan_columns(ctx, prog, lits, t0, t1, &cp));
    BlobOffsets offs{};
    bool fresh_blob = false;
    SPK_TRY(upload_program(ctx, prog, lits, cp, &offs, &fresh_blob));
#ifdef SPK_HOST_TIMING
    const auto ht2 = std::chrono::steady_clock::now();
#endif
    const WindowLayout L = layout_windows(ctx, cp.long_exact);
    const int n_slots = L.split ? 2 : 1;
    SPK_TRY(alloc_slots(ctx, L, cp.C, n_slots));
    GammaArgs A = gamma_args(ctx, t0, t1, cp, offs);
    const int64_t img_stride = cp.img_stride;
    if (!ctx->gcols) ctx->gcols = new GammaCols();
    *ctx->gcols = std::move(cp.C);  // kept for the settlement (settle_gammas), which may come after this call
    const GammaCols &C = *ctx->gcols;
    ctx->last_simple = (int)C.simple.size();
    ctx->exact_carry.clear();
    ctx->deferred_carry = 0;
    ctx->last_windows = L.n_win;
    ctx->last_slots = n_slots;
    SPK_TRY(ctx->begin(K_GAMMA));
    // row images and rule-view images: kernels only when a table, the column layout or the pairs changed
    ViewLaunch V{};
    bool have_view = false;
    if (L.P > 0) {
        SPK_TRY(build_images(ctx, t0, t1, A, img_stride, C.simple));
        // regions wholly inside rule 1's pairs read its view-ordered image (view launch); the others, and a
        // region straddling a rule boundary, the table image (table launches).  Only when the image
        // outgrows the caches: at 1M rows (80 MB, held by the 256 MB Infinity Cache) the second launch's
        // tail cost 4 % (1.41 vs 1.34 ms, cfg2); at 20M rows (1.6 GB) the view launch took the pass from
        // 31.1 to 22.8 ms (profiles/archive/r2_ab_views.log).
        const bool big = (A.img_rows0 + A.img_rows1) * img_stride > VIEW_MIN_IMAGE_BYTES;
        if ((ctx->use_views == 1 && big) || ctx->use_views == 2) SPK_TRY(build_view_images(ctx, A, img_stride, &V, &have_view));
    }
    const GammaRun R{A, L, have_view ? &V : nullptr};
    bool via_graph = false;
    SPK_TRY(run_pass(ctx, R, fresh_blob, &via_graph));
    SPK_TRY(ctx->end(K_GAMMA));
    for (int i = 0; i < n_slots; ++i) {
        // the info blocks on the context stream behind the pass (a split call without a graph read each window's
        // back on its own stream)
        if (!L.split || via_graph) SPK_TRY(read_info(ctx, ctx->slot[i], ctx->stream));
        ctx->slot[i].gamma_pending = true;
    }
    ++ctx->gamma_seq;
    ctx->codes_valid = true;
    ctx->mpat_valid = false;
    ctx->last_implied.assign((size_t)C.K, 0);
    for (const SimpleCol &sc : C.simple) ctx->last_implied[sc.k] = sc.imp_hi - sc.imp_lo;
#ifdef SPK_HOST_TIMING
    {  // diagnostic build only: host time per spk_gammas phase (settle wait, program preparation, enqueue)
        static double acc[3] = {0, 0, 0};
        static int calls = 0;
        const auto ht3 = std::chrono::steady_clock::now();
        acc[0] += std::chrono::duration<double, std::micro>(ht1 - ht0).count();
        acc[1] += std::chrono::duration<double, std::micro>(ht2 - ht1).count();
        acc[2] += std::chrono::duration<double, std::micro>(ht3 - ht2).count();
        if (++calls % 20 == 0) {
            std::fprintf(stderr, "[spk host] per call: settle %.1f us, prepare %.1f us, enqueue %.1f us\n", acc[0] / 20,
                         acc[1] / 20, acc[2] / 20);
            acc[0] = acc[1] = acc[2] = 0;
        }
    }
#endif
    return SPK_OK;
}

extern "C" int spk_gammas_load(spk_ctx *ctx, int n_cols, const int32_t *n_levels, int64_t n, const int8_t *gammas) {
    SPK_REQUIRE(ctx && n_levels && n >= 0 && (n == 0 || gammas), SPK_E_INVALID, "spk_gammas_load: bad args");
    SPK_HIP(hipSetDevice(ctx->device));
    SPK_TRY(settle_gammas(ctx, nullptr));
    SPK_TRY(set_pattern_space(ctx, n_cols, n_levels));
    for (int64_t p = 0; p < n; ++p)
        for (int k = 0; k < n_cols; ++k)
            SPK_REQUIRE(gammas[p * n_cols + k] >= -1 && gammas[p * n_cols + k] < n_levels[k], SPK_E_INVALID,
                        "spk_gammas_load: gamma value out of range");
    DevBuf<int8_t> d_g;
    DevBuf<int64_t> d_stride;
    SPK_TRY(d_g.alloc((size_t)n * n_cols + 1));
    SPK_TRY(d_stride.alloc((size_t)n_cols));
    if (n) SPK_HIP(hipMemcpyAsync(d_g.p, gammas, (size_t)n * n_cols, hipMemcpyHostToDevice, ctx->stream));
    SPK_HIP(hipMemcpyAsync(d_stride.p, ctx->stride.data(), (size_t)n_cols * 8, hipMemcpyHostToDevice, ctx->stream));
    SPK_TRY(ctx->codes.alloc((size_t)(n + 1) * ctx->code_bytes));
    if (n) {
        k_codes_from_gammas<<<(unsigned)((n + 255) / 256), 256, 0, ctx->stream>>>(n, n_cols, d_g.p, d_stride.p,
                                                                              ctx->codes.p, ctx->code_bytes);
        SPK_HIP(hipGetLastError());
    }
    SPK_HIP(hipStreamSynchronize(ctx->stream));
    ctx->n_pairs = n;
    for (Slot &S : ctx->slot) S.gamma_pending = false;
    ++ctx->gamma_seq;
    ctx->codes_valid = true;
    return SPK_OK;
}

extern "C" int spk_gammas_copy(spk_ctx *ctx, int64_t start, int64_t count, int8_t *out) {
    SPK_REQUIRE(ctx && out, SPK_E_INVALID, "spk_gammas_copy: bad args");
    SPK_REQUIRE(ctx->codes_valid, SPK_E_STATE, "spk_gammas_copy: no gammas");
    SPK_REQUIRE(start >= 0 && count >= 0 && start + count <= ctx->n_pairs, SPK_E_INVALID, "range out of bounds");
    SPK_HIP(hipSetDevice(ctx->device));
    SPK_TRY(settle_gammas(ctx, nullptr));
    if (!count) return SPK_OK;
    DevBuf<int8_t> d_out;
    DevBuf<int64_t> d_stride;
    DevBuf<int32_t> d_nlev;
    SPK_TRY(d_out.alloc((size_t)count * ctx->K));
    SPK_TRY(d_stride.alloc((size_t)ctx->K));
    SPK_TRY(d_nlev.alloc((size_t)ctx->K));
    SPK_HIP(hipMemcpyAsync(d_stride.p, ctx->stride.data(), (size_t)ctx->K * 8, hipMemcpyHostToDevice, ctx->stream));
    SPK_HIP(hipMemcpyAsync(d_nlev.p, ctx->n_levels.data(), (size_t)ctx->K * 4, hipMemcpyHostToDevice, ctx->stream));
    k_gammas_from_codes<<<(unsigned)((count + 255) / 256), 256, 0, ctx->stream>>>(
        start, count, ctx->K, ctx->codes.p, ctx->code_bytes, d_stride.p, d_nlev.p, d_out.p);
    SPK_HIP(hipGetLastError());
    SPK_HIP(hipMemcpyAsync(out, d_out.p, (size_t)count * ctx->K, hipMemcpyDeviceToHost, ctx->stream));
    SPK_HIP(hipStreamSynchronize(ctx->stream));
    return SPK_OK;
}

extern "C" int spk_n_patterns(spk_ctx *ctx, int64_t *out) {
    SPK_REQUIRE(ctx && out, SPK_E_INVALID, "null arg");
    *out = ctx->n_patterns;
    return SPK_OK;
}

extern "C" int spk_gammas_exact_ms(spk_ctx *ctx, double *out, int n) {
    SPK_REQUIRE(ctx && out && n >= 0, SPK_E_INVALID, "spk_gammas_exact_ms: bad args");
    SPK_HIP(hipSetDevice(ctx->device));
    SPK_TRY(settle_gammas(ctx, nullptr));
    SPK_HIP(hipStreamSynchronize(ctx->stream));
    // every window of the call timed its launch on its own stream: the sum over the slots the call used
    for (int k = 0; k < n; ++k) {
        out[k] = -1.0;
        for (int i = 0; i < ctx->last_slots; ++i) {
            const Slot &S = ctx->slot[i];
            if (k >= (int)S.xev_used.size() || !S.xev_used[k]) continue;
            float ms = 0.f;
            SPK_HIP(hipEventElapsedTime(&ms, S.xev0[k], S.xev1[k]));
            out[k] = (out[k] < 0 ? 0.0 : out[k]) + (double)ms;
        }
    }
    return SPK_OK;
}

extern "C" int spk_gammas_deferred(spk_ctx *ctx, int64_t *out) {
    SPK_REQUIRE(ctx && out, SPK_E_INVALID, "null arg");
    SPK_TRY(settle_gammas(ctx, nullptr));
    *out = ctx->last_deferred;
    return SPK_OK;
}

extern "C" int spk_gammas_exact_list(spk_ctx *ctx, int k, int32_t *out, int64_t n) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "null ctx");
    SPK_TRY(settle_gammas(ctx, nullptr));
    SPK_REQUIRE(out && k >= 0 && k < (int)ctx->last_exact.size() && n >= 0, SPK_E_INVALID,
                "spk_gammas_exact_list: bad args");
    // the lists carried from the windows settled during the call, then each slot the call used: its window's list;
    // the window-relative ordinals made global
    int64_t done = 0;
    auto take = [&](const int32_t *list, int64_t count, int64_t first) -> int {
        const int64_t m = std::min<int64_t>(n - done, count);
        if (m <= 0) return SPK_OK;
        SPK_HIP(hipMemcpy(out + done, list, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (int64_t j = done; j < done + m; ++j)
            if (out[j] >= 0) out[j] += (int32_t)first;
        done += m;
        return SPK_OK;
    };
    for (const spk_ctx::ListSeg &g : ctx->list_carry)
        if (g.k == k) SPK_TRY(take(ctx->xcarry.p + g.off, g.n, g.first));
    for (int i = 0; i < ctx->last_slots; ++i) {
        const Slot &S = ctx->slot[i];
        const GammaPlan &G = *S.gplan;
        if (k < (int)G.exact.size()) SPK_TRY(take(S.xlist.p + G.xbase[k], G.exact[k], G.first));
    }
    return SPK_OK;
}

extern "C" int spk_gammas_exact_counts(spk_ctx *ctx, int64_t *out, int n) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "null ctx");
    SPK_TRY(settle_gammas(ctx, nullptr));
    SPK_REQUIRE(out && n >= (int)ctx->last_exact.size(), SPK_E_INVALID, "spk_gammas_exact_counts: bad args");
    for (size_t k = 0; k < ctx->last_exact.size(); ++k) out[k] = ctx->last_exact[k];
    return SPK_OK;
}

extern "C" int spk_gammas_implied_pairs(spk_ctx *ctx, int64_t *out, int n) {
    SPK_REQUIRE(ctx && out && n >= (int)ctx->last_implied.size(), SPK_E_INVALID, "spk_gammas_implied_pairs: bad args");
    for (size_t k = 0; k < ctx->last_implied.size(); ++k) out[k] = ctx->last_implied[k];
    return SPK_OK;
}

extern "C" int spk_gammas_set_simple(spk_ctx *ctx, int on) {
    SPK_REQUIRE(ctx && on >= 0 && on % 10 <= 1 && on % 100 < 30 && on < 200, SPK_E_INVALID,
                "spk_gammas_set_simple: mode 0, 1 (+10 / +20) (+100)");
    ctx->use_views = on % 100 >= 20 ? 2 : (on % 100 >= 10 ? 0 : 1);
    ctx->filter_mode = on % 10;
    ctx->slow_force_skip = on >= 100;
    return SPK_OK;
}

extern "C" int spk_gammas_view_regions(spk_ctx *ctx, int64_t *out) {
    SPK_REQUIRE(ctx && out, SPK_E_INVALID, "null arg");
    *out = ctx->last_view_regions;
    return SPK_OK;
}

extern "C" int spk_gammas_simple_count(spk_ctx *ctx, int *out) {
    SPK_REQUIRE(ctx && out, SPK_E_INVALID, "null arg");
    *out = ctx->last_simple;
    return SPK_OK;
}

extern "C" int spk_gammas_set_window(spk_ctx *ctx, int64_t pairs) {
    SPK_REQUIRE(ctx && pairs >= 0, SPK_E_INVALID, "spk_gammas_set_window: bad args");
    ctx->gamma_window = pairs;
    return SPK_OK;
}

extern "C" int spk_gammas_set_graph(spk_ctx *ctx, int on) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "null ctx");
    ctx->use_graph = on != 0;
    ctx->gkey_prev.clear();
    return SPK_OK;
}

extern "C" int spk_gammas_graph_launches(spk_ctx *ctx, int64_t *out) {
    SPK_REQUIRE(ctx && out, SPK_E_INVALID, "null arg");
    *out = ctx->graph_launches;
    return SPK_OK;
}

extern "C" int spk_gammas_set_streams(spk_ctx *ctx, int streams, int64_t min_pairs) {
    SPK_REQUIRE(ctx && (streams == 1 || streams == 2) && min_pairs >= 0, SPK_E_INVALID,
                "spk_gammas_set_streams: 1 or 2 streams, min_pairs >= 0");
    SPK_TRY(settle_gammas(ctx, nullptr));
    ctx->gamma_streams = streams;
    ctx->split_min = min_pairs;
    return SPK_OK;
}

extern "C" int spk_gammas_windows(spk_ctx *ctx, int64_t *out) {
    SPK_REQUIRE(ctx && out, SPK_E_INVALID, "spk_gammas_windows: bad args");
    *out = ctx->last_windows;
    return SPK_OK;
}

extern "C" int spk_gammas_set_lev_kernel(spk_ctx *ctx, int mode) {
    SPK_REQUIRE(ctx && mode >= 0 && mode <= 3, SPK_E_INVALID, "spk_gammas_set_lev_kernel: mode 0 .. 3");
    ctx->lev_kernel = mode == 3 ? 2 : mode;
    ctx->lev_bag = mode != 3;
    return SPK_OK;
}

extern "C" int spk_gammas_set_lev_bound(spk_ctx *ctx, int mode) {
    SPK_REQUIRE(ctx && (mode == 0 || mode == 1), SPK_E_INVALID, "spk_gammas_set_lev_bound: mode 0 or 1");
    ctx->lev_bound = mode;  // SimpleCol.pos follows it: the next spk_gammas lays the row image out again
    return SPK_OK;
}
