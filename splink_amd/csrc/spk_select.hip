// Selection of scored pairs (gfx950): df_e.filter("match_probability > t and gamma_x >= 1") on the device.
//
// A pair's match_probability and every gamma are functions of its packed comparison code, so a conjunction of
// comparisons over them is decided once per pattern: k_select_patterns writes a keep bitset over the pattern
// space.  Per pair the work is one bit lookup and a stable compaction: k_select<EMIT = false> counts the kept
// pairs of every chunk of SEL_CHUNK ordinals, the counts are scanned (CountScan), and k_select<EMIT = true>
// writes each survivor's ordinal, rows and code at chunk offset + kept pairs before it, the order of the
// ordinals.  Nothing of P elements is allocated but the chunk counts, and no fp64 is written for a dropped pair;
// levels and match_probability are decoded from the survivors' codes when they are copied out.
//
// A chunk belongs to one wave, so the ranks need no LDS and no barrier: a lane loads 16 bytes of codes (8 or 4
// pairs) per slab, the wave's lanes hold consecutive pairs, and for element j of every lane one ballot gives the
// kept pairs of the slab at that element; a pair's position is the popcounts of those ballots below its lane plus
// the kept elements before it in its own lane.
//
// spk_select_tf* adds terms on tf_adjusted_match_prob, which is a function of the pair's code (through mp) and of its
// two rows (through the tf value ids), so it is decided per pair, as a cascade: the pattern stage above is unchanged
// and a pair whose pattern fails it gathers nothing; k_select_tf_count evaluates the tf terms of the pattern-kept
// pairs (tf_pair's arithmetic, spk_tf_pair.h), counts, and writes one 64-bit ballot word per (chunk, slab, element):
// a keep bitmap of P / 8 bytes.  k_select_tf_emit takes the ranks from those words and recomputes
// tf_adjusted_match_prob and the adjustments for the survivors only.
//
// spk_select_sample keeps, per stratum of match_probability, the quota pairs with the smallest counter-based random
// keys: the stratum is a function of the pattern (a byte per pattern beside the keep bit's logic), the thresholds come
// from a radix select over the keys that stores nothing per pair, and the survivors from the same count, scan and emit
// (see "spk_select_sample" below).
//
// spk_select_top keeps the first k eligible pairs in score order (NULL lowest, ties by ordinal): the score is a function
// of the pattern, so the cut is found on the pattern table by a weighted radix select, a byte per pattern says above the
// cut / at the cut / out, and the count, scan and emit run with two counts per chunk; spk_select_top_of does the same
// over a selection's survivors and their stored scores (see "spk_select_top" below).
#include <algorithm>
#include <cmath>

#include "spk_prim.h"
#include "spk_tf_pair.h"

namespace spk {

constexpr int SEL_THREADS = 256;
constexpr int SEL_WAVES = SEL_THREADS / 64;
constexpr int64_t SEL_CHUNK = 2048;     // pair ordinals per count (one wave's work item); _native.SELECT_CHUNK mirrors it
constexpr int SEL_WG_PER_CU = 8;        // capped grid, the waves stride over the chunks (as k_score)
constexpr int64_t SEL_LDS_PAT = 1 << 18;  // keep bitset in LDS up to this many patterns (32 KiB)
constexpr int SEL_MAXK = 64;            // PatArgs' column limit

typedef uint32_t sel_u32x4 __attribute__((ext_vector_type(4)));
typedef int32_t sel_i32x4 __attribute__((ext_vector_type(4)));

struct SelPatArgs {
    int K, n_terms;
    int64_t n_pat;
    int32_t stride[SEL_MAXK];
    uint8_t nlev[SEL_MAXK];
    spk_select_term terms[SPK_SELECT_MAX_TERMS];
};

// SQL three-valued comparison of v with x: a NULL v (null = true) is TRUE only under IS NULL.  NE is written as
// "less or greater", so a NaN on either side gives false where C's != would give true.
__device__ inline bool sel_term_true(int op, bool null, double v, double x) {
    switch (op) {
        case SPK_SEL_IS_NULL: return null;
        case SPK_SEL_IS_NOT_NULL: return !null;
        case SPK_SEL_LT: return !null && v < x;
        case SPK_SEL_LE: return !null && v <= x;
        case SPK_SEL_GT: return !null && v > x;
        case SPK_SEL_GE: return !null && v >= x;
        case SPK_SEL_EQ: return !null && v == x;
        case SPK_SEL_NE: return !null && (v < x || v > x);
        default: return false;
    }
}

// The conjunction of A's terms for pattern p < n_pat: the levels the terms read are decoded with PatArgs' strides.
__device__ inline bool sel_pattern_true(const SelPatArgs &A, const double *__restrict__ mpat, int64_t p) {
    bool k = true;
    for (int t = 0; t < A.n_terms; ++t) {
        const spk_select_term T = A.terms[t];
        bool null = false;
        double v;
        if (T.field == SPK_SEL_MP) {
            v = mpat[p];
            null = v != v;
        } else {
            v = (double)((int)((p / A.stride[T.col]) % (A.nlev[T.col] + 1)) - 1);
        }
        k = k && sel_term_true(T.op, null, v, T.value);
    }
    return k;
}

// One thread per pattern: evaluate the conjunction, and write the wave's 64 keep bits as one word.  keep has
// (n_pat + 63) / 64 words; mpat may be null (no SPK_SEL_MP term).
__global__ __launch_bounds__(SEL_THREADS) void k_select_patterns(SelPatArgs A, const double *__restrict__ mpat,
                                                                 unsigned long long *__restrict__ keep) {
    const int64_t p = (int64_t)blockIdx.x * SEL_THREADS + threadIdx.x;
    const bool k = p < A.n_pat && sel_pattern_true(A, mpat, p);
    const unsigned long long m = __ballot(k);
    if ((threadIdx.x & 63) == 0 && (p >> 6) < (A.n_pat + 63) / 64) keep[p >> 6] = m;
}

struct SelectArgs {
    const void *codes;          // uint16 or uint32, one per pair
    int64_t P, n_chunks;
    const uint32_t *keep;       // the bitset as 32-bit words
    int64_t n_pat;
    int keep_words;             // 32-bit words staged in LDS (LDS form)
    const int32_t *pl, *pr;     // the pairs' rows, or null (no pair set)
    int64_t *chunk_count;       // count pass output
    const int64_t *chunk_off;   // emit pass input [n_chunks + 1]
    int64_t *out_ord;
    int32_t *out_l, *out_r;
    uint32_t *out_code;
};

// The codes of the chunk at ordinal `base`, 16 bytes per lane and slab (lane's pairs are consecutive).
template <typename CodeT>
__device__ inline void sel_load_chunk(const CodeT *__restrict__ codes, int64_t base, int64_t P, int lane,
                                      sel_u32x4 (&v)[SEL_CHUNK / (64 * (16 / (int)sizeof(CodeT)))]) {
    constexpr int V = 16 / (int)sizeof(CodeT);
    constexpr int SLABS = (int)(SEL_CHUNK / (64 * V));
    if (base + SEL_CHUNK <= P) {  // whole chunk: every lane's 16 bytes lie inside the codes (wave-uniform)
        const sel_u32x4 *src = reinterpret_cast<const sel_u32x4 *>(codes + base);
#pragma unroll
        for (int s = 0; s < SLABS; ++s) v[s] = __builtin_nontemporal_load(src + s * 64 + lane);
    } else {  // the last chunk: code by code, zero past the end (masked out by the ordinal where it is used)
#pragma unroll
        for (int s = 0; s < SLABS; ++s) {
            uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const int64_t p = base + ((int64_t)s * 64 + lane) * V + j;
                const uint32_t x = p < P ? (uint32_t)codes[p] : 0u;
                if (sizeof(CodeT) == 2) w[j >> 1] |= x << (16 * (j & 1));
                else w[j] = x;
            }
            v[s] = sel_u32x4{w[0], w[1], w[2], w[3]};
        }
    }
}

// Code j of a lane's slab vector.
template <typename CodeT>
__device__ inline uint32_t sel_code(const sel_u32x4 &v, int j) {
    return sizeof(CodeT) == 2 ? (v[j >> 1] >> (16 * (j & 1))) & 0xFFFFu : v[j];
}

template <typename CodeT, bool LDS, bool EMIT>
__global__ __launch_bounds__(SEL_THREADS) void k_select(SelectArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_keep[];
    if (LDS) {
        for (int i = threadIdx.x; i < A.keep_words; i += SEL_THREADS) s_keep[i] = A.keep[i];
        __syncthreads();
    }
    const uint32_t *T = LDS ? s_keep : A.keep;
    constexpr int V = 16 / (int)sizeof(CodeT);            // codes per lane and slab
    constexpr int SLABS = (int)(SEL_CHUNK / (64 * V));    // slabs per chunk
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    const CodeT *codes = reinterpret_cast<const CodeT *>(A.codes);
    const int64_t n_waves = (int64_t)gridDim.x * SEL_WAVES;
    for (int64_t c = (int64_t)blockIdx.x * SEL_WAVES + wave; c < A.n_chunks; c += n_waves) {
        int64_t run = 0;
        if (EMIT) {
            run = A.chunk_off[c];
            if (A.chunk_off[c + 1] == run) continue;  // nothing kept here (wave-uniform)
        }
        const int64_t base = c * SEL_CHUNK;
        sel_u32x4 v[SLABS];
        sel_load_chunk<CodeT>(codes, base, A.P, lane, v);
        int wave_total = 0;
#pragma unroll
        for (int s = 0; s < SLABS; ++s) {
            const int64_t p0 = base + ((int64_t)s * 64 + lane) * V;  // this lane's first pair of the slab
            uint32_t code[V];
            unsigned km = 0;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const uint32_t x = sel_code<CodeT>(v[s], j);
                code[j] = x;
                const bool k = p0 + j < A.P && (int64_t)x < A.n_pat && ((T[x >> 5] >> (x & 31u)) & 1u);
                km |= (k ? 1u : 0u) << j;
            }
            int before = 0, all = 0;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const unsigned long long m = __ballot((km >> j) & 1u);
                all += __popcll(m);
                before += __popcll(m & below);
            }
            if (!EMIT) {
                wave_total += all;
                continue;
            }
            int64_t q = run + before;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                if ((km >> j) & 1u) {
                    const int64_t p = p0 + j;
                    A.out_ord[q] = p;
                    A.out_code[q] = code[j];
                    if (A.pl) {
                        A.out_l[q] = A.pl[p];
                        A.out_r[q] = A.pr[p];
                    }
                    ++q;
                }
            }
            run += all;
        }
        if (!EMIT && lane == 0) A.chunk_count[c] = wave_total;
    }
}

// What the tf kernels need beyond SelectArgs: the call's id arrays and tables, the selection's own mp per pattern
// (never ctx->mp), the SPK_SEL_TF_MP terms, the keep bitmap and the survivors' tf outputs.
struct SelTfArgs {
    TfApply T;
    const double *mpat;
    int n_terms;
    int32_t op[SPK_SELECT_MAX_TERMS];
    double value[SPK_SELECT_MAX_TERMS];
    unsigned long long *bitmap;  // [n_chunks x SEL_CHUNK / 64]: word (chunk, slab, element) = the ballot of its 64 pairs
    double *out_tf, *out_adj;    // emit pass: [n_sel], [n_sel x T.n]
};

// The pattern-kept pairs of a lane's slab as a mask over its V elements (k_select's test).
template <typename CodeT>
__device__ inline unsigned sel_pattern_mask(const sel_u32x4 &v, int64_t p0, int64_t P, int64_t n_pat,
                                            const uint32_t *__restrict__ T, uint32_t (&code)[16 / (int)sizeof(CodeT)]) {
    constexpr int V = 16 / (int)sizeof(CodeT);
    unsigned km = 0;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const uint32_t x = sel_code<CodeT>(v, j);
        code[j] = x;
        const bool k = p0 + j < P && (int64_t)x < n_pat && ((T[x >> 5] >> (x & 31u)) & 1u);
        km |= (k ? 1u : 0u) << j;
    }
    return km;
}

// Count pass with tf terms.  Chunk, slab and lane layout of k_select.  A slab none of whose pairs passed the
// pattern stage gathers nothing; otherwise the lanes load their pairs' rows (consecutive: 16-byte vectors), and for
// the pattern-kept pairs, column by column, the value ids of every element, then the table entries, then the fold:
// the loads of all elements are issued before the first is used.  One ballot per element gives the chunk count and
// the bitmap word.
template <typename CodeT, bool LDS>
__global__ __launch_bounds__(SEL_THREADS) void k_select_tf_count(SelectArgs A, SelTfArgs F) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_keep[];
    if (LDS) {
        for (int i = threadIdx.x; i < A.keep_words; i += SEL_THREADS) s_keep[i] = A.keep[i];
        __syncthreads();
    }
    const uint32_t *T = LDS ? s_keep : A.keep;
    constexpr int V = 16 / (int)sizeof(CodeT);
    constexpr int SLABS = (int)(SEL_CHUNK / (64 * V));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const CodeT *codes = reinterpret_cast<const CodeT *>(A.codes);
    const int64_t n_waves = (int64_t)gridDim.x * SEL_WAVES;
    for (int64_t c = (int64_t)blockIdx.x * SEL_WAVES + wave; c < A.n_chunks; c += n_waves) {
        const int64_t base = c * SEL_CHUNK;
        const bool whole = base + SEL_CHUNK <= A.P;  // wave-uniform
        unsigned long long *words = F.bitmap + c * (SEL_CHUNK / 64);
        sel_u32x4 v[SLABS];
        sel_load_chunk<CodeT>(codes, base, A.P, lane, v);
        int wave_total = 0;
#pragma unroll
        for (int s = 0; s < SLABS; ++s) {
            const int64_t p0 = base + ((int64_t)s * 64 + lane) * V;  // this lane's first pair of the slab
            uint32_t code[V];
            const unsigned km = sel_pattern_mask<CodeT>(v[s], p0, A.P, A.n_pat, T, code);
            if (__ballot(km != 0u) == 0ull) {  // wave-uniform: nothing to gather
                if (lane == 0) {
#pragma unroll
                    for (int j = 0; j < V; ++j) words[s * V + j] = 0ull;
                }
                continue;
            }
            int32_t l[V], r[V];
#pragma unroll
            for (int j = 0; j < V; ++j) l[j] = r[j] = 0;
            if (km != 0u) {
                if (whole) {  // p0 is a multiple of V >= 4: 16-byte aligned, and p0 + V <= P
                    const sel_i32x4 *L = reinterpret_cast<const sel_i32x4 *>(A.pl + p0);
                    const sel_i32x4 *R = reinterpret_cast<const sel_i32x4 *>(A.pr + p0);
#pragma unroll
                    for (int q = 0; q < V / 4; ++q) {
                        const sel_i32x4 xl = __builtin_nontemporal_load(L + q), xr = __builtin_nontemporal_load(R + q);
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            l[4 * q + e] = xl[e];
                            r[4 * q + e] = xr[e];
                        }
                    }
                } else {  // the last chunk: a kept element lies below P
#pragma unroll
                    for (int j = 0; j < V; ++j)
                        if ((km >> j) & 1u) {
                            l[j] = __builtin_nontemporal_load(A.pl + p0 + j);
                            r[j] = __builtin_nontemporal_load(A.pr + p0 + j);
                        }
                }
            }
            double m[V], a[V], b[V];
#pragma unroll
            for (int j = 0; j < V; ++j) {
                m[j] = (km >> j) & 1u ? F.mpat[code[j]] : 0.0;  // code < n_pat: the pattern mask checked it
                tf_begin(m[j], a[j], b[j]);
            }
            for (int t = 0; t < F.T.n; ++t) {
                const int64_t *__restrict__ i0 = F.T.ids0[t];
                const int64_t *__restrict__ i1 = F.T.ids1[t];
                const double *__restrict__ tab = F.T.tab[t];
                const int64_t tab_n = F.T.tab_n[t];
                int64_t ia[V], ib[V];
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    ia[j] = ib[j] = -1;
                    if ((km >> j) & 1u) {
                        ia[j] = i0[l[j]];
                        ib[j] = i1[r[j]];
                    }
                }
                double x[V];
#pragma unroll
                for (int j = 0; j < V; ++j) x[j] = tf_adj(ia[j], ib[j], tab, tab_n);  // -1: no load
#pragma unroll
                for (int j = 0; j < V; ++j) tf_fold(a[j], b[j], x[j]);
            }
            unsigned kt = 0;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const double tf = tf_finish(m[j], a[j], b[j]);
                bool k = (km >> j) & 1u;
                for (int t = 0; t < F.n_terms; ++t) k = k && sel_term_true(F.op[t], tf != tf, tf, F.value[t]);
                kt |= (k ? 1u : 0u) << j;
            }
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const unsigned long long w = __ballot((kt >> j) & 1u);
                wave_total += __popcll(w);
                if (lane == 0) words[s * V + j] = w;
            }
        }
        if (lane == 0) A.chunk_count[c] = wave_total;
    }
}

// Emit pass of a selection with tf tables: k_select's outputs, and for the survivors tf_adjusted_match_prob and the
// adjustments, recomputed with tf_pair.  BITMAP: the kept pairs are the count pass's bitmap words (there were tf
// terms); otherwise the pattern bitset decides, as in k_select.
template <typename CodeT, bool LDS, bool BITMAP>
__global__ __launch_bounds__(SEL_THREADS) void k_select_tf_emit(SelectArgs A, SelTfArgs F) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_keep[];
    if (LDS && !BITMAP) {
        for (int i = threadIdx.x; i < A.keep_words; i += SEL_THREADS) s_keep[i] = A.keep[i];
        __syncthreads();
    }
    const uint32_t *T = LDS ? s_keep : A.keep;
    constexpr int V = 16 / (int)sizeof(CodeT);
    constexpr int SLABS = (int)(SEL_CHUNK / (64 * V));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    const CodeT *codes = reinterpret_cast<const CodeT *>(A.codes);
    const int64_t n_waves = (int64_t)gridDim.x * SEL_WAVES;
    for (int64_t c = (int64_t)blockIdx.x * SEL_WAVES + wave; c < A.n_chunks; c += n_waves) {
        int64_t run = A.chunk_off[c];
        if (A.chunk_off[c + 1] == run) continue;  // nothing kept here (wave-uniform)
        const int64_t base = c * SEL_CHUNK;
        const unsigned long long *words = BITMAP ? F.bitmap + c * (SEL_CHUNK / 64) : nullptr;
        sel_u32x4 v[SLABS];
        sel_load_chunk<CodeT>(codes, base, A.P, lane, v);
#pragma unroll
        for (int s = 0; s < SLABS; ++s) {
            const int64_t p0 = base + ((int64_t)s * 64 + lane) * V;
            uint32_t code[V];
            unsigned km = 0;
            int before = 0, all = 0;
            if (BITMAP) {
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    code[j] = sel_code<CodeT>(v[s], j);
                    const unsigned long long w = words[s * V + j];
                    km |= (unsigned)((w >> lane) & 1ull) << j;
                    all += __popcll(w);
                    before += __popcll(w & below);
                }
            } else {
                km = sel_pattern_mask<CodeT>(v[s], p0, A.P, A.n_pat, T, code);
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const unsigned long long w = __ballot((km >> j) & 1u);
                    all += __popcll(w);
                    before += __popcll(w & below);
                }
            }
            int64_t q = run + before;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                if ((km >> j) & 1u) {
                    const int64_t p = p0 + j;
                    const int32_t l = __builtin_nontemporal_load(A.pl + p), r = __builtin_nontemporal_load(A.pr + p);
                    A.out_ord[q] = p;
                    A.out_code[q] = code[j];
                    A.out_l[q] = l;
                    A.out_r[q] = r;
                    F.out_tf[q] = tf_pair(F.T, F.mpat[code[j]], l, r, F.out_adj + q * F.T.n);
                    ++q;
                }
            }
            run += all;
        }
    }
}

struct SelDecodeArgs {
    int64_t start, count;
    int K;
    const uint32_t *code;
    const double *mpat;   // or null
    int8_t *out_g;        // [count x K] or null
    double *out_mp;       // or null
    int32_t stride[SEL_MAXK];
    uint8_t nlev[SEL_MAXK];
};

// Survivors [start, start + count): levels from the code (spk_gammas' packing), mp from the selection's table.
__global__ __launch_bounds__(256) void k_select_decode(SelDecodeArgs A) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.count) return;
    const int64_t c = A.code[A.start + i];
    if (A.out_g)
        for (int k = 0; k < A.K; ++k) A.out_g[i * A.K + k] = (int8_t)((int)((c / A.stride[k]) % (A.nlev[k] + 1)) - 1);
    if (A.out_mp) A.out_mp[i] = A.mpat[c];
}

// ---- spk_select_sample: per stratum of match_probability, the quota[b] eligible pairs with the smallest keys ----
// The stratum is a function of the pattern, like the keep bit: k_sample_patterns writes one byte per pattern (SMP_NONE:
// fails a term, NULL score, or outside the edges).  The quota[b]-th smallest key of every stratum is found by a radix
// select, most significant digit first, with nothing stored per pair: pass d of k_sample<SMP_HIST> streams the codes in
// k_select's chunk layout, recomputes each pair's key from its ordinal, and counts digit d of the keys that agree with
// their stratum's prefix in the digits above it, into an LDS histogram [n_strata][256] that is added to the global one
// at the end; k_sample_pick (one workgroup) then takes, per stratum, the digit at which the running count reaches what
// is left of the quota, extends the prefix by it and reduces the remainder by the count below it.  After 8 passes the
// prefix is the threshold: exactly quota[b] keys of the stratum are <= it.  A stratum with population <= quota is
// settled in pass 0 (threshold all ones: kept whole), so is quota 0 (none kept), and once no stratum is left the later
// histogram passes return at their first load.  Histograms are integer sums, so nothing depends on arrival order.
// k_sample<SMP_COUNT> and <SMP_EMIT> are k_select's two passes under `in a stratum and key <= its threshold`.
constexpr int SMP_MAX = SPK_SAMPLE_MAX_STRATA;
constexpr int SMP_NONE = 255;                  // the stratum byte of a pattern that is never sampled
constexpr int SMP_DIGITS = 256, SMP_PASSES = 8;  // 8 bits per pass over the 64-bit key
constexpr int SMP_WG_PER_CU = 2;               // histogram passes: fewer workgroups, fewer histograms to add up
constexpr int64_t SMP_LDS_BYTES = 80 * 1024;   // two workgroups of a CU's 160 KiB stay resident: the histogram (64 KiB at
                                               // 64 strata) and, while it fits beside it, the stratum table
constexpr int64_t SMP_STATIC_BYTES = 1024;     // reserved for k_sample's static LDS (s_key, s_flag)
static_assert(SMP_MAX < SMP_NONE && SMP_MAX % SEL_WAVES == 0, "stratum byte, k_sample_pick's strata per wave");

// The per-stratum state of one call, 64-bit words on the device: [ST_x + b] for stratum b.
enum { ST_PREFIX = 0, ST_REMAIN = SMP_MAX, ST_THR = 2 * SMP_MAX, ST_FLAG = 3 * SMP_MAX, ST_POP = 4 * SMP_MAX,
       ST_KEPT = 5 * SMP_MAX, ST_ACTIVE = 6 * SMP_MAX, ST_WORDS = 6 * SMP_MAX + 1 };
enum { SMP_ACTIVE = 0, SMP_ALL = 1, SMP_EMPTY = 2 };  // ST_FLAG: still selecting / kept whole / none kept

// spk_sample.hip's sm_mix, restated (spk_select_sample's keys are part of the ABI: the values must not change).
__host__ __device__ inline uint64_t smp_mix(uint64_t x) {
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}
__device__ inline uint64_t smp_key(uint64_t seed_mix, int64_t p) {
    return smp_mix(seed_mix + 0x9E3779B97F4A7C15ull * ((uint64_t)p + 1ull));
}

struct SmpPatArgs {
    int n_strata;
    double edges[SMP_MAX + 1];
};

// One thread per pattern: its stratum, or SMP_NONE.  tab [n_pat]; mpat is the call's mp table (never null).
__global__ __launch_bounds__(SEL_THREADS) void k_sample_patterns(SelPatArgs A, SmpPatArgs E,
                                                                 const double *__restrict__ mpat,
                                                                 uint8_t *__restrict__ tab) {
    const int64_t p = (int64_t)blockIdx.x * SEL_THREADS + threadIdx.x;
    if (p >= A.n_pat) return;
    const double x = mpat[p];
    int b = SMP_NONE;
    // a NaN fails both comparisons; the last stratum is closed on the right, so edges[n_strata] is no boundary below
    if (x >= E.edges[0] && x <= E.edges[E.n_strata] && sel_pattern_true(A, mpat, p)) {
        b = 0;
        for (int i = 1; i < E.n_strata; ++i) b += x >= E.edges[i] ? 1 : 0;
    }
    tab[p] = (uint8_t)b;
}

enum { SMP_HIST = 0, SMP_COUNT = 1, SMP_EMIT = 2 };

struct SmpArgs {
    const void *codes;          // uint16 or uint32, one per pair
    int64_t P, n_chunks;
    const uint8_t *tab;         // stratum per pattern
    int64_t n_pat;
    int tab_words;              // 32-bit words of tab staged in LDS (LDS form)
    int n_strata, pass;         // pass: SMP_HIST's digit, 0 = the most significant
    uint64_t seed_mix;          // mix(seed)
    const unsigned long long *st;  // the strata's state (SMP_HIST: read from pass 1 on)
    unsigned long long *hist;   // SMP_HIST: [n_strata x SMP_DIGITS], zero at launch
    const int32_t *pl, *pr;     // as SelectArgs from here on
    int64_t *chunk_count;
    const int64_t *chunk_off;
    int64_t *out_ord;
    int32_t *out_l, *out_r;
    uint32_t *out_code;
};

template <typename CodeT, bool LDS, int MODE>
__global__ __launch_bounds__(SEL_THREADS) void k_sample(SmpArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_dyn[];  // SMP_HIST: the histogram; then the table (LDS)
    __shared__ unsigned long long s_key[SMP_MAX];  // SMP_HIST: the stratum's prefix; otherwise its threshold
    __shared__ int s_flag[SMP_MAX];
    if (MODE == SMP_HIST && A.pass > 0 && A.st[ST_ACTIVE] == 0ull) return;  // every stratum is settled (grid-uniform)
    const int hist_words = MODE == SMP_HIST ? A.n_strata * SMP_DIGITS : 0;
    uint32_t *s_hist = s_dyn;
    uint32_t *s_tab = s_dyn + hist_words;
    for (int i = threadIdx.x; i < hist_words; i += SEL_THREADS) s_hist[i] = 0u;
    if (LDS)
        for (int i = threadIdx.x; i < A.tab_words; i += SEL_THREADS)
            s_tab[i] = reinterpret_cast<const uint32_t *>(A.tab)[i];
    const bool state = MODE != SMP_HIST || A.pass > 0;  // pass 0 counts every pair in a stratum
    if (state && threadIdx.x < A.n_strata) {
        s_key[threadIdx.x] = A.st[(MODE == SMP_HIST ? ST_PREFIX : ST_THR) + threadIdx.x];
        s_flag[threadIdx.x] = (int)A.st[ST_FLAG + threadIdx.x];
    }
    __syncthreads();
    const uint8_t *T = LDS ? reinterpret_cast<const uint8_t *>(s_tab) : A.tab;
    constexpr int V = 16 / (int)sizeof(CodeT);            // codes per lane and slab
    constexpr int SLABS = (int)(SEL_CHUNK / (64 * V));    // slabs per chunk
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int digit_shift = 56 - 8 * A.pass;  // SMP_HIST: the digit; the bits above it are digit_shift + 8 .. 63
    const CodeT *codes = reinterpret_cast<const CodeT *>(A.codes);
    const int64_t n_waves = (int64_t)gridDim.x * SEL_WAVES;
    for (int64_t c = (int64_t)blockIdx.x * SEL_WAVES + wave; c < A.n_chunks; c += n_waves) {
        int64_t run = 0;
        if (MODE == SMP_EMIT) {
            run = A.chunk_off[c];
            if (A.chunk_off[c + 1] == run) continue;  // nothing kept here (wave-uniform)
        }
        const int64_t base = c * SEL_CHUNK;
        sel_u32x4 v[SLABS];
        sel_load_chunk<CodeT>(codes, base, A.P, lane, v);
        int wave_total = 0;
#pragma unroll
        for (int s = 0; s < SLABS; ++s) {
            const int64_t p0 = base + ((int64_t)s * 64 + lane) * V;  // this lane's first pair of the slab
            uint32_t code[V];
            unsigned km = 0;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const uint32_t x = sel_code<CodeT>(v[s], j);
                code[j] = x;
                const int b = p0 + j < A.P && (int64_t)x < A.n_pat ? (int)T[x] : SMP_NONE;
                if (b >= A.n_strata) continue;  // SMP_NONE
                const uint64_t key = smp_key(A.seed_mix, p0 + j);
                if (MODE == SMP_HIST) {
                    // digit_shift + 8 is 16 .. 56 here: pass 0 reads no state
                    const bool in = !state || (s_flag[b] == SMP_ACTIVE &&
                                               (key >> (digit_shift + 8)) == (s_key[b] >> (digit_shift + 8)));
                    if (in) atomicAdd(&s_hist[b * SMP_DIGITS + (int)((key >> digit_shift) & 255u)], 1u);
                } else {
                    km |= (s_flag[b] != SMP_EMPTY && key <= s_key[b] ? 1u : 0u) << j;
                }
            }
            if (MODE == SMP_HIST) continue;
            int before = 0, all = 0;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const unsigned long long m = __ballot((km >> j) & 1u);
                all += __popcll(m);
                before += __popcll(m & below);
            }
            if (MODE == SMP_COUNT) {
                wave_total += all;
                continue;
            }
            int64_t q = run + before;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                if ((km >> j) & 1u) {
                    const int64_t p = p0 + j;
                    A.out_ord[q] = p;
                    A.out_code[q] = code[j];
                    if (A.pl) {
                        A.out_l[q] = A.pl[p];
                        A.out_r[q] = A.pr[p];
                    }
                    ++q;
                }
            }
            run += all;
        }
        if (MODE == SMP_COUNT && lane == 0) A.chunk_count[c] = wave_total;
    }
    if (MODE == SMP_HIST) {  // a workgroup's count of a bin fits 32 bits: it sees at most n_chunks / gridDim.x + 1 chunks
        __syncthreads();
        for (int i = threadIdx.x; i < hist_words; i += SEL_THREADS) {
            const uint32_t n = s_hist[i];
            if (n) atomicAdd(&A.hist[i], (unsigned long long)n);
        }
    }
}

struct SmpPickArgs {
    int n_strata, pass;
    unsigned long long *hist;  // [n_strata x SMP_DIGITS] of this pass; left zero for the next
    unsigned long long *st;
    int64_t quota[SMP_MAX];
};

// One workgroup, a wave per stratum at a time, a lane per 4 digits.  Pass 0 also settles population, kept count and
// the strata that need no selecting.  For an active stratum, 1 <= remainder <= the keys under its prefix, so exactly one
// lane's digits contain the remainder-th key.
__global__ __launch_bounds__(SEL_THREADS) void k_sample_pick(SmpPickArgs A) {
    __shared__ int s_active;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_active = 0;
    __syncthreads();
    for (int r = 0; r < SMP_MAX / SEL_WAVES; ++r) {
        const int b = r * SEL_WAVES + wave;
        if (b >= A.n_strata) break;  // wave-uniform
        unsigned long long *h = A.hist + (size_t)b * SMP_DIGITS + 4 * lane;
        unsigned long long c[4], own = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            c[j] = h[j];
            h[j] = 0ull;
            own += c[j];
        }
        unsigned long long incl = own;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long t = __shfl_up(incl, d);
            if (lane >= d) incl += t;
        }
        const unsigned long long total = __shfl(incl, 63);
        unsigned long long k;
        int flag;
        if (A.pass == 0) {
            k = (unsigned long long)A.quota[b] < total ? (unsigned long long)A.quota[b] : total;
            flag = k == 0ull ? SMP_EMPTY : k == total ? SMP_ALL : SMP_ACTIVE;
            if (lane == 0) {
                A.st[ST_POP + b] = total;
                A.st[ST_KEPT + b] = k;
                A.st[ST_FLAG + b] = (unsigned long long)flag;
                A.st[ST_THR + b] = ~0ull;
                if (flag == SMP_ACTIVE) atomicAdd(&s_active, 1);
            }
        } else {
            flag = (int)A.st[ST_FLAG + b];
            k = A.st[ST_REMAIN + b];
        }
        if (flag != SMP_ACTIVE) continue;  // wave-uniform
        unsigned long long before = incl - own;
        if (before < k && k <= incl) {
            int j = 0;
            while (j < 3 && before + c[j] < k) before += c[j++];
            const unsigned long long prefix =
                (A.pass == 0 ? 0ull : A.st[ST_PREFIX + b]) | ((unsigned long long)(4 * lane + j) << (56 - 8 * A.pass));
            A.st[ST_PREFIX + b] = prefix;
            A.st[ST_REMAIN + b] = k - before;
            if (A.pass == SMP_PASSES - 1) A.st[ST_THR + b] = prefix;
        }
    }
    __syncthreads();
    if (A.pass == 0 && threadIdx.x == 0) A.st[ST_ACTIVE] = (unsigned long long)s_active;
}

// The grid of every per-pair kernel here: capped, the waves stride over the chunks.
static unsigned select_grid(spk_ctx *ctx, int64_t n_chunks) {
    int64_t g = (n_chunks + SEL_WAVES - 1) / SEL_WAVES;
    return (unsigned)std::max<int64_t>(std::min<int64_t>(g, SEL_WG_PER_CU * (int64_t)ctx->n_cu), 1);
}

template <typename CodeT, bool EMIT>
static int launch_select(spk_ctx *ctx, const SelectArgs &A, bool lds) {
    const unsigned g = select_grid(ctx, A.n_chunks);
    if (lds) k_select<CodeT, true, EMIT><<<g, SEL_THREADS, (size_t)A.keep_words * 4, ctx->stream>>>(A);
    else k_select<CodeT, false, EMIT><<<g, SEL_THREADS, 0, ctx->stream>>>(A);
    SPK_HIP(hipGetLastError());
    return SPK_OK;
}

template <bool EMIT>
static int launch_select_codes(spk_ctx *ctx, const SelectArgs &A, bool lds) {
    return ctx->code_bytes == 2 ? launch_select<uint16_t, EMIT>(ctx, A, lds) : launch_select<uint32_t, EMIT>(ctx, A, lds);
}

template <typename CodeT>
static int launch_tf_count(spk_ctx *ctx, const SelectArgs &A, const SelTfArgs &F, bool lds) {
    const unsigned g = select_grid(ctx, A.n_chunks);
    if (lds) k_select_tf_count<CodeT, true><<<g, SEL_THREADS, (size_t)A.keep_words * 4, ctx->stream>>>(A, F);
    else k_select_tf_count<CodeT, false><<<g, SEL_THREADS, 0, ctx->stream>>>(A, F);
    SPK_HIP(hipGetLastError());
    return SPK_OK;
}

template <typename CodeT>
static int launch_tf_emit(spk_ctx *ctx, const SelectArgs &A, const SelTfArgs &F, bool lds, bool bitmap) {
    const unsigned g = select_grid(ctx, A.n_chunks);
    if (bitmap) k_select_tf_emit<CodeT, false, true><<<g, SEL_THREADS, 0, ctx->stream>>>(A, F);
    else if (lds) k_select_tf_emit<CodeT, true, false><<<g, SEL_THREADS, (size_t)A.keep_words * 4, ctx->stream>>>(A, F);
    else k_select_tf_emit<CodeT, false, false><<<g, SEL_THREADS, 0, ctx->stream>>>(A, F);
    SPK_HIP(hipGetLastError());
    return SPK_OK;
}

// What every selection records of the context it is taken from: the pattern space, whether the pairs have rows, and
// the counters that say when it goes stale.
static void selection_header(spk_ctx *ctx, bool has_mp, Selection &S) {
    const size_t P = (size_t)ctx->n_pairs;
    S.K = ctx->K;
    S.n_levels = ctx->n_levels;
    S.stride = ctx->stride;
    S.has_mp = has_mp;
    S.has_rows = ctx->pairs_valid && ctx->pl.p && ctx->pr.p && ctx->pl.n >= P && ctx->pr.n >= P;
    S.pairs_epoch = ctx->pairs_epoch;
    S.gamma_seq = ctx->gamma_seq;
    S.fix_seq = ctx->codes_fix_seq;
}

// The emit pass's outputs for n_sel survivors.
static int selection_alloc(Selection &S, int64_t n_sel) {
    SPK_TRY(S.ord.alloc((size_t)n_sel + 1));
    SPK_TRY(S.code.alloc((size_t)n_sel + 1));
    if (S.has_rows) {
        SPK_TRY(S.l.alloc((size_t)n_sel + 1));
        SPK_TRY(S.r.alloc((size_t)n_sel + 1));
    }
    return SPK_OK;
}

// The selection into S (a local of spk_select*: a failure on the way leaves the context without one).  tf: the staged
// id arrays and tables of spk_select_tf* (the SPK_SEL_TF_MP terms are evaluated per pair, the others per pattern), or
// null for spk_select.
static int build_selection(spk_ctx *ctx, double lambda, double one_minus, const double *m, const double *u, int n_terms,
                           const spk_select_term *terms, const TfApply *tf, Selection &S) {
    const int64_t P = ctx->n_pairs, n_pat = ctx->n_patterns;
    const int K = ctx->K;
    SelPatArgs PA{};
    SelTfArgs F{};
    PA.K = K;
    PA.n_pat = n_pat;
    for (int k = 0; k < K; ++k) {
        PA.stride[k] = (int32_t)ctx->stride[k];
        PA.nlev[k] = (uint8_t)ctx->n_levels[k];
    }
    for (int t = 0; t < n_terms; ++t) {
        if (terms[t].field == SPK_SEL_TF_MP) {
            F.op[F.n_terms] = terms[t].op;
            F.value[F.n_terms++] = terms[t].value;
        } else {
            PA.terms[PA.n_terms++] = terms[t];
        }
    }
    const bool tf_terms = F.n_terms > 0;
    if (tf) {
        F.T = *tf;
        S.has_tf = true;
        S.n_tf = tf->n;
    }
    selection_header(ctx, m && u, S);
    StageTimer T{ctx};
    const int64_t words64 = (n_pat + 63) / 64;
    DevBuf<unsigned long long> keep;
    DevBuf<uint8_t> tmp;
    CountScan chunks;
    DevBuf<unsigned long long> bitmap;  // per-pair keep bits of the tf count pass: P / 8 bytes, gone at return
    SPK_TRY(keep.alloc((size_t)words64 + 1));
    if (S.has_mp) SPK_TRY(S.mpat.alloc((size_t)n_pat + 1));
    const int64_t n_chunks = (P + SEL_CHUNK - 1) / SEL_CHUNK;
    SPK_TRY(chunks.alloc(ctx, n_chunks));
    if (tf_terms) SPK_TRY(bitmap.alloc((size_t)(n_chunks * (SEL_CHUNK / 64)) + 1));
    F.mpat = S.mpat.p;
    F.bitmap = bitmap.p;
    // ---- per pattern: mp table, keep bitset; per chunk: the kept pairs; their scan
    SPK_TRY(T.open());
    if (S.has_mp) SPK_TRY(pattern_mp_table(ctx, lambda, one_minus, m, u, S.mpat.p));
    if (n_pat > 0) {
        k_select_patterns<<<(unsigned)((n_pat + SEL_THREADS - 1) / SEL_THREADS), SEL_THREADS, 0, ctx->stream>>>(
            PA, S.mpat.p, keep.p);
        SPK_HIP(hipGetLastError());
    }
    SelectArgs A{};
    A.codes = ctx->codes.p;
    A.P = P;
    A.n_chunks = n_chunks;
    A.keep = reinterpret_cast<const uint32_t *>(keep.p);
    A.n_pat = n_pat;
    A.keep_words = (int)std::min<int64_t>(2 * words64, INT32_MAX);
    A.pl = S.has_rows ? ctx->pl.p : nullptr;
    A.pr = S.has_rows ? ctx->pr.p : nullptr;
    const bool lds = n_pat <= SEL_LDS_PAT;
    if (n_chunks > 0) {
        A.chunk_count = chunks.count.p;
        if (!tf_terms) SPK_TRY(launch_select_codes<false>(ctx, A, lds));
        else if (ctx->code_bytes == 2) SPK_TRY(launch_tf_count<uint16_t>(ctx, A, F, lds));
        else SPK_TRY(launch_tf_count<uint32_t>(ctx, A, F, lds));
    }
    SPK_TRY(scan_total(ctx, chunks, tmp, &T));  // synchronises
    const int64_t n_sel = chunks.total;
    SPK_REQUIRE(n_sel >= 0 && n_sel <= P, SPK_E_STATE, "spk_select: survivor count");
    // ---- the survivors
    SPK_TRY(selection_alloc(S, n_sel));
    if (tf) {
        SPK_TRY(S.tf_mp.alloc((size_t)n_sel + 1));
        SPK_TRY(S.adj.alloc((size_t)n_sel * tf->n + 1));
        F.out_tf = S.tf_mp.p;
        F.out_adj = S.adj.p;
    }
    if (n_sel > 0) {
        A.chunk_count = nullptr;
        A.chunk_off = chunks.off.p;
        A.out_ord = S.ord.p;
        A.out_code = S.code.p;
        A.out_l = S.l.p;
        A.out_r = S.r.p;
        SPK_TRY(T.open());
        if (!tf) SPK_TRY(launch_select_codes<true>(ctx, A, lds));
        else if (ctx->code_bytes == 2) SPK_TRY(launch_tf_emit<uint16_t>(ctx, A, F, lds, tf_terms));
        else SPK_TRY(launch_tf_emit<uint32_t>(ctx, A, F, lds, tf_terms));
        SPK_TRY(T.close());
    }
    S.n = n_sel;
    S.ms = T.result();
    S.valid = true;
    return SPK_OK;
}

template <typename CodeT, int MODE>
static int launch_sample(spk_ctx *ctx, const SmpArgs &A, bool lds) {
    const int64_t cap = (MODE == SMP_HIST ? SMP_WG_PER_CU : SEL_WG_PER_CU) * (int64_t)ctx->n_cu;
    const int64_t g = std::max<int64_t>(std::min<int64_t>((A.n_chunks + SEL_WAVES - 1) / SEL_WAVES, cap), 1);
    // a workgroup's 32-bit LDS counters: the pairs its waves see
    const int64_t per_wg = ((A.n_chunks + g * SEL_WAVES - 1) / (g * SEL_WAVES)) * SEL_WAVES * SEL_CHUNK;
    SPK_REQUIRE(MODE != SMP_HIST || per_wg < ((int64_t)1 << 32), SPK_E_LIMIT, "spk_select_sample: too many pairs");
    const size_t bytes = (MODE == SMP_HIST ? (size_t)A.n_strata * SMP_DIGITS * 4 : 0) + (lds ? (size_t)A.tab_words * 4 : 0);
    if (lds) k_sample<CodeT, true, MODE><<<(unsigned)g, SEL_THREADS, bytes, ctx->stream>>>(A);
    else k_sample<CodeT, false, MODE><<<(unsigned)g, SEL_THREADS, bytes, ctx->stream>>>(A);
    SPK_HIP(hipGetLastError());
    return SPK_OK;
}

template <int MODE>
static int launch_sample_codes(spk_ctx *ctx, const SmpArgs &A, bool lds) {
    return ctx->code_bytes == 2 ? launch_sample<uint16_t, MODE>(ctx, A, lds) : launch_sample<uint32_t, MODE>(ctx, A, lds);
}

// spk_select_sample's selection into S, and the strata's eligible and kept pairs into pop / kept [n_strata].  One host
// round trip, build_selection's: the strata's counts come back with the scan's total.
static int build_sample(spk_ctx *ctx, double lambda, double one_minus, const double *m, const double *u, int n_terms,
                        const spk_select_term *terms, int n_strata, const double *edges, const int64_t *quota,
                        uint64_t seed, Selection &S, std::vector<int64_t> &pop, std::vector<int64_t> &kept) {
    const int64_t P = ctx->n_pairs, n_pat = ctx->n_patterns;
    SelPatArgs PA{};
    SmpPatArgs E{};
    SmpPickArgs K{};
    PA.K = ctx->K;
    PA.n_pat = n_pat;
    for (int k = 0; k < ctx->K; ++k) {
        PA.stride[k] = (int32_t)ctx->stride[k];
        PA.nlev[k] = (uint8_t)ctx->n_levels[k];
    }
    for (int t = 0; t < n_terms; ++t) PA.terms[PA.n_terms++] = terms[t];
    E.n_strata = K.n_strata = n_strata;
    for (int b = 0; b <= n_strata; ++b) E.edges[b] = edges[b];
    for (int b = 0; b < n_strata; ++b) K.quota[b] = quota[b];
    selection_header(ctx, true, S);
    const int64_t hist_bytes = (int64_t)n_strata * SMP_DIGITS * 4, tab_bytes = (n_pat + 3) / 4 * 4;
    const int64_t budget = std::min<int64_t>(SMP_LDS_BYTES, ctx->lds_per_block) - SMP_STATIC_BYTES;
    SPK_REQUIRE(hist_bytes <= budget, SPK_E_LIMIT, "spk_select_sample: the strata's histogram exceeds the device's LDS");
    const bool lds = hist_bytes + tab_bytes <= budget;
    StageTimer T{ctx};
    DevBuf<uint8_t> tab, tmp;
    DevBuf<unsigned long long> hist, st;
    CountScan chunks;
    SPK_TRY(tab.alloc((size_t)tab_bytes + 4));
    SPK_TRY(hist.alloc((size_t)n_strata * SMP_DIGITS));
    SPK_TRY(st.alloc(ST_WORDS));
    SPK_TRY(S.mpat.alloc((size_t)n_pat + 1));
    const int64_t n_chunks = (P + SEL_CHUNK - 1) / SEL_CHUNK;
    SPK_TRY(chunks.alloc(ctx, n_chunks));
    K.hist = hist.p;
    K.st = st.p;
    // ---- per pattern: mp table, stratum; the strata's thresholds; per chunk: the kept pairs; their scan
    SPK_TRY(T.open());
    SPK_HIP(hipMemsetAsync(tab.p, SMP_NONE, (size_t)tab_bytes + 4, ctx->stream));
    SPK_HIP(hipMemsetAsync(hist.p, 0, (size_t)n_strata * SMP_DIGITS * 8, ctx->stream));
    SPK_HIP(hipMemsetAsync(st.p, 0, (size_t)ST_WORDS * 8, ctx->stream));
    SPK_TRY(pattern_mp_table(ctx, lambda, one_minus, m, u, S.mpat.p));
    if (n_pat > 0) {
        k_sample_patterns<<<(unsigned)((n_pat + SEL_THREADS - 1) / SEL_THREADS), SEL_THREADS, 0, ctx->stream>>>(
            PA, E, S.mpat.p, tab.p);
        SPK_HIP(hipGetLastError());
    }
    SmpArgs A{};
    A.codes = ctx->codes.p;
    A.P = P;
    A.n_chunks = n_chunks;
    A.tab = tab.p;
    A.n_pat = n_pat;
    A.tab_words = (int)(tab_bytes / 4);
    A.n_strata = n_strata;
    A.seed_mix = smp_mix(seed);
    A.st = st.p;
    A.hist = hist.p;
    A.pl = S.has_rows ? ctx->pl.p : nullptr;
    A.pr = S.has_rows ? ctx->pr.p : nullptr;
    for (int pass = 0; pass < SMP_PASSES; ++pass) {
        A.pass = K.pass = pass;
        if (n_chunks > 0) SPK_TRY(launch_sample_codes<SMP_HIST>(ctx, A, lds));
        k_sample_pick<<<1, SEL_THREADS, 0, ctx->stream>>>(K);
        SPK_HIP(hipGetLastError());
    }
    A.pass = 0;
    if (n_chunks > 0) {
        A.chunk_count = chunks.count.p;
        SPK_TRY(launch_sample_codes<SMP_COUNT>(ctx, A, lds));
    }
    std::vector<unsigned long long> counts(2 * SMP_MAX);  // ST_POP and ST_KEPT are adjacent
    SPK_HIP(hipMemcpyAsync(counts.data(), st.p + ST_POP, counts.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    SPK_TRY(scan_total(ctx, chunks, tmp, &T));  // synchronises
    const int64_t n_sel = chunks.total;
    int64_t want = 0;
    pop.assign(n_strata, 0);
    kept.assign(n_strata, 0);
    for (int b = 0; b < n_strata; ++b) {
        pop[b] = (int64_t)counts[b];
        kept[b] = (int64_t)counts[SMP_MAX + b];
        want += kept[b];
    }
    SPK_REQUIRE(n_sel == want && n_sel <= P, SPK_E_STATE, "spk_select_sample: survivor count");
    // ---- the survivors
    SPK_TRY(selection_alloc(S, n_sel));
    if (n_sel > 0) {
        A.chunk_count = nullptr;
        A.chunk_off = chunks.off.p;
        A.out_ord = S.ord.p;
        A.out_code = S.code.p;
        A.out_l = S.l.p;
        A.out_r = S.r.p;
        SPK_TRY(T.open());
        SPK_TRY(launch_sample_codes<SMP_EMIT>(ctx, A, lds));
        SPK_TRY(T.close());
    }
    S.n = n_sel;
    S.ms = T.result();
    S.valid = true;
    return SPK_OK;
}

// ---- spk_select_top / spk_select_top_of: the first k eligible pairs in score order ----
// Both orders become "smallest key first": top_key maps a score to an unsigned 64-bit key that is monotone in the
// order asked for (NULL = NaN lowest ascending, so last descending; -0.0 and +0.0 share a key).  A radix select, most
// significant byte first, finds the key of the k-th element: pass d counts digit d of the keys that agree with the
// prefix in the digits above it (256 integer bins; the order of the atomics does not matter), and k_top_pick (one
// wave) takes the digit at which the running count reaches what is left of k, extends the prefix by it and reduces the
// remainder by the count below it.  After 8 passes the prefix is the cut key, the remainder is how many elements at
// the cut are kept, and the chosen bin's count is how many there are.  Pass 0 also settles the total, and k = 0 or
// k >= total (nothing to select: none or all kept), after which the later histogram passes return at once.
//   spk_select_top: the score is a function of the pattern, so the elements are the eligible patterns, weighted by
//     their pairs (k_top_hist: one pass over the codes), and a byte per pattern (k_top_classes) says above the cut, at
//     the cut or out.  k_top<EMIT = false> counts both classes per chunk, both counts are scanned, and k_top<EMIT =
//     true> emits the pairs above the cut and the pairs at the cut whose exclusive rank among the at-the-cut pairs, in
//     ordinal order across the chunks, is below the remainder: a chunk's output starts at (above before it) +
//     min(at the cut before it, remainder).
//   spk_select_top_of: the elements are the selection's survivors with their stored scores (k_topof_hist), and
//     k_topof<EMIT> is the same two-count compaction over them, in spk_select_best's chunk layout.
// SPK_TOP_FIRST is the same compaction with every eligible pair at the cut and remainder k; no score is read.
enum { TOP_OUT = 0, TOP_ABOVE = 1, TOP_AT = 2 };                               // a pattern's / survivor's class
enum { TS_PREFIX = 0, TS_REMAIN, TS_FLAG, TS_TOTAL, TS_TIED, TS_WORDS };      // the call's state, 64-bit device words
enum { TOP_ACTIVE = 0, TOP_ALL = 1, TOP_EMPTY = 2, TOP_FIRSTK = 3 };          // TS_FLAG
constexpr int TOP_DIGITS = 256, TOP_PASSES = 8;
constexpr int64_t TOP_LDS_HIST = 8192;    // k_top_hist: 32-bit counters in LDS up to this many patterns (32 KiB)
constexpr int64_t TOP_LDS_TAB = 32768;    // k_top: the class bytes in LDS up to this many patterns (32 KiB)
constexpr int TOP_PAT_WG_PER_CU = 4;

__host__ __device__ inline unsigned long long top_key(double s, bool desc) {
    unsigned long long img = 0ull;  // NULL
    if (s == s) {
        unsigned long long u;
#if defined(__HIP_DEVICE_COMPILE__)
        u = (unsigned long long)__double_as_longlong(s);
#else
        __builtin_memcpy(&u, &s, 8);
#endif
        if ((u << 1) == 0ull) u = 0ull;  // -0.0 -> +0.0
        img = (u >> 63) ? ~u : (u | 0x8000000000000000ull);  // never 0: -inf is 0x000F...F
    }
    return desc ? ~img : img;
}

// The score a key stands for (NaN: NULL).
static double top_key_score(unsigned long long key, bool desc) {
    const unsigned long long img = desc ? ~key : key;
    if (img == 0ull) return __builtin_nan("");
    const unsigned long long u = (img >> 63) ? (img & 0x7FFFFFFFFFFFFFFFull) : ~img;
    double s;
    __builtin_memcpy(&s, &u, 8);
    return s;
}

__device__ inline int top_class(int flag, unsigned long long cut, unsigned long long key) {
    if (flag == TOP_ALL) return TOP_ABOVE;
    if (flag == TOP_EMPTY) return TOP_OUT;
    if (flag == TOP_FIRSTK) return TOP_AT;
    return key < cut ? TOP_ABOVE : key == cut ? TOP_AT : TOP_OUT;
}

// The pairs per pattern: hist [n_pat], zero at launch.  k_select's chunk layout.  LDS: 32-bit counters per workgroup,
// added to the global ones at the end (a workgroup sees fewer than 2^32 pairs: launch_top_hist checks).
template <typename CodeT, bool LDS>
__global__ __launch_bounds__(SEL_THREADS) void k_top_hist(const void *codes_, int64_t P, int64_t n_chunks, int64_t n_pat,
                                                          unsigned long long *__restrict__ hist) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_cnt[];
    if (LDS) {
        for (int i = threadIdx.x; i < (int)n_pat; i += SEL_THREADS) s_cnt[i] = 0u;
        __syncthreads();
    }
    constexpr int V = 16 / (int)sizeof(CodeT);
    constexpr int SLABS = (int)(SEL_CHUNK / (64 * V));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const CodeT *codes = reinterpret_cast<const CodeT *>(codes_);
    const int64_t n_waves = (int64_t)gridDim.x * SEL_WAVES;
    for (int64_t c = (int64_t)blockIdx.x * SEL_WAVES + wave; c < n_chunks; c += n_waves) {
        const int64_t base = c * SEL_CHUNK;
        sel_u32x4 v[SLABS];
        sel_load_chunk<CodeT>(codes, base, P, lane, v);
#pragma unroll
        for (int s = 0; s < SLABS; ++s) {
            const int64_t p0 = base + ((int64_t)s * 64 + lane) * V;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                // one pattern holds most pairs (every column disagrees): the lanes whose code is the first lane's are
                // counted with one ballot and added once, so a hot counter sees one atomic per wave, not 64
                const uint32_t x = sel_code<CodeT>(v[s], j);
                const bool valid = p0 + j < P && (int64_t)x < n_pat;
                const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)x);
                const bool same = valid && x == first;
                const unsigned long long m = __ballot(same);
                if (valid && (!same || lane == __ffsll((long long)m) - 1)) {
                    const uint32_t n = same ? (uint32_t)__popcll(m) : 1u;
                    if (LDS) atomicAdd(&s_cnt[x], n);
                    else atomicAdd(&hist[x], (unsigned long long)n);
                }
            }
        }
    }
    if (LDS) {
        __syncthreads();
        for (int i = threadIdx.x; i < (int)n_pat; i += SEL_THREADS) {
            const uint32_t n = s_cnt[i];
            if (n) atomicAdd(&hist[i], (unsigned long long)n);
        }
    }
}

struct TopPatArgs {
    int64_t n_pat;
    const unsigned long long *keep;  // the eligible patterns (k_select_patterns)
    const unsigned long long *cnt;   // pairs per pattern (k_top_hist)
    const double *mpat;
    int desc, pass;
    unsigned long long *hist;        // [TOP_DIGITS], zero at launch
    const unsigned long long *st;
};

// Pass `pass` of the weighted select: digit `pass` of the eligible patterns' keys under the prefix, weighted by their
// pairs.  The workgroups stride over the patterns.
__global__ __launch_bounds__(SEL_THREADS) void k_top_pat_hist(TopPatArgs A) {
    __shared__ unsigned long long s_h[TOP_DIGITS];
    if (A.pass > 0 && A.st[TS_FLAG] != (unsigned long long)TOP_ACTIVE) return;  // settled (grid-uniform)
    for (int i = threadIdx.x; i < TOP_DIGITS; i += SEL_THREADS) s_h[i] = 0ull;
    __syncthreads();
    const unsigned long long prefix = A.pass > 0 ? A.st[TS_PREFIX] : 0ull;
    const int shift = 56 - 8 * A.pass;  // the bits above the digit are shift + 8 .. 63 (pass 0: none)
    for (int64_t p = (int64_t)blockIdx.x * SEL_THREADS + threadIdx.x; p < A.n_pat; p += (int64_t)gridDim.x * SEL_THREADS) {
        if (!((A.keep[p >> 6] >> (p & 63)) & 1ull)) continue;
        const unsigned long long w = A.cnt[p];
        if (w == 0ull) continue;
        const unsigned long long key = top_key(A.mpat[p], A.desc != 0);
        if (A.pass > 0 && (key >> (shift + 8)) != (prefix >> (shift + 8))) continue;
        atomicAdd(&s_h[(int)((key >> shift) & 255ull)], w);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < TOP_DIGITS; i += SEL_THREADS) {
        const unsigned long long n = s_h[i];
        if (n) atomicAdd(&A.hist[i], n);
    }
}

// One wave, a lane per 4 digits (k_sample_pick for one stratum with quota k).  While active, 1 <= remainder <= the
// elements under the prefix, so exactly one lane's digits contain the remainder-th element.  Leaves hist zero.
__global__ __launch_bounds__(64) void k_top_pick(unsigned long long *__restrict__ hist, unsigned long long *__restrict__ st,
                                                 int64_t k, int pass) {
    const int lane = threadIdx.x;
    unsigned long long c[4], own = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        c[j] = hist[4 * lane + j];
        hist[4 * lane + j] = 0ull;
        own += c[j];
    }
    unsigned long long incl = own;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long t = __shfl_up(incl, d);
        if (lane >= d) incl += t;
    }
    const unsigned long long total = __shfl(incl, 63);
    unsigned long long rem, prefix = 0ull;
    int flag;
    if (pass == 0) {
        rem = (unsigned long long)k < total ? (unsigned long long)k : total;
        flag = rem == 0ull ? TOP_EMPTY : rem == total ? TOP_ALL : TOP_ACTIVE;
        if (lane == 0) {
            st[TS_TOTAL] = total;
            st[TS_FLAG] = (unsigned long long)flag;
        }
    } else {
        flag = (int)st[TS_FLAG];
        rem = st[TS_REMAIN];
        prefix = st[TS_PREFIX];
    }
    if (flag != TOP_ACTIVE) return;  // wave-uniform
    unsigned long long before = incl - own;
    if (before < rem && rem <= incl) {
        int j = 0;
        while (j < 3 && before + c[j] < rem) before += c[j++];
        st[TS_PREFIX] = prefix | ((unsigned long long)(4 * lane + j) << (56 - 8 * pass));
        st[TS_REMAIN] = rem - before;
        if (pass == TOP_PASSES - 1) st[TS_TIED] = c[j];
    }
}

// One thread per pattern: its class byte.  mpat may be null under TOP_FIRSTK (no score is read).
__global__ __launch_bounds__(SEL_THREADS) void k_top_classes(int64_t n_pat, const unsigned long long *__restrict__ keep,
                                                             const double *__restrict__ mpat, int desc,
                                                             const unsigned long long *__restrict__ st,
                                                             uint8_t *__restrict__ tab) {
    const int64_t p = (int64_t)blockIdx.x * SEL_THREADS + threadIdx.x;
    if (p >= n_pat) return;
    const int flag = (int)st[TS_FLAG];
    int cls = TOP_OUT;
    if ((keep[p >> 6] >> (p & 63)) & 1ull)
        cls = top_class(flag, st[TS_PREFIX], flag == TOP_ACTIVE ? top_key(mpat[p], desc != 0) : 0ull);
    tab[p] = (uint8_t)cls;
}

struct TopArgs {
    const void *codes;          // uint16 or uint32, one per pair
    int64_t P, n_chunks;
    const uint8_t *tab;         // class per pattern
    int64_t n_pat;
    int tab_words;              // 32-bit words of tab staged in LDS (LDS form)
    int64_t r;                  // emit pass: the at-the-cut pairs kept
    const int32_t *pl, *pr;     // the pairs' rows, or null (no pair set)
    int64_t *above_count, *at_count;        // count pass output
    const int64_t *above_off, *at_off;      // emit pass input [n_chunks + 1]
    int64_t *out_ord;
    int32_t *out_l, *out_r;
    uint32_t *out_code;
};

__device__ inline int64_t top_min(int64_t a, int64_t b) { return a < b ? a : b; }

template <typename CodeT, bool LDS, bool EMIT>
__global__ __launch_bounds__(SEL_THREADS) void k_top(TopArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_tab[];
    if (LDS) {
        for (int i = threadIdx.x; i < A.tab_words; i += SEL_THREADS) s_tab[i] = reinterpret_cast<const uint32_t *>(A.tab)[i];
        __syncthreads();
    }
    const uint8_t *T = LDS ? reinterpret_cast<const uint8_t *>(s_tab) : A.tab;
    constexpr int V = 16 / (int)sizeof(CodeT);            // codes per lane and slab
    constexpr int SLABS = (int)(SEL_CHUNK / (64 * V));    // slabs per chunk
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    const CodeT *codes = reinterpret_cast<const CodeT *>(A.codes);
    const int64_t n_waves = (int64_t)gridDim.x * SEL_WAVES;
    for (int64_t c = (int64_t)blockIdx.x * SEL_WAVES + wave; c < A.n_chunks; c += n_waves) {
        int64_t run = 0, at_run = 0;
        if (EMIT) {
            at_run = A.at_off[c];
            run = A.above_off[c] + top_min(at_run, A.r);
            if (A.above_off[c + 1] + top_min(A.at_off[c + 1], A.r) == run) continue;  // nothing kept here (wave-uniform)
        }
        const int64_t base = c * SEL_CHUNK;
        sel_u32x4 v[SLABS];
        sel_load_chunk<CodeT>(codes, base, A.P, lane, v);
        int n_above = 0, n_at = 0;
#pragma unroll
        for (int s = 0; s < SLABS; ++s) {
            const int64_t p0 = base + ((int64_t)s * 64 + lane) * V;  // this lane's first pair of the slab
            uint32_t code[V];
            unsigned am = 0, tm = 0;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const uint32_t x = sel_code<CodeT>(v[s], j);
                code[j] = x;
                const int cls = p0 + j < A.P && (int64_t)x < A.n_pat ? (int)T[x] : TOP_OUT;
                am |= (cls == TOP_ABOVE ? 1u : 0u) << j;
                tm |= (cls == TOP_AT ? 1u : 0u) << j;
            }
            int at_before = 0, at_all = 0;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const unsigned long long m = __ballot((tm >> j) & 1u);
                at_all += __popcll(m);
                at_before += __popcll(m & below);
            }
            if (!EMIT) {
#pragma unroll
                for (int j = 0; j < V; ++j) n_above += __popcll(__ballot((am >> j) & 1u));
                n_at += at_all;
                continue;
            }
            unsigned km = am;
            int64_t rank = at_run + at_before;  // at-the-cut pairs before this lane's first, over the whole pair set
#pragma unroll
            for (int j = 0; j < V; ++j) {
                if ((tm >> j) & 1u) {
                    if (rank < A.r) km |= 1u << j;
                    ++rank;
                }
            }
            int before = 0, all = 0;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const unsigned long long m = __ballot((km >> j) & 1u);
                all += __popcll(m);
                before += __popcll(m & below);
            }
            int64_t q = run + before;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                if ((km >> j) & 1u) {
                    const int64_t p = p0 + j;
                    A.out_ord[q] = p;
                    A.out_code[q] = code[j];
                    if (A.pl) {
                        A.out_l[q] = A.pl[p];
                        A.out_r[q] = A.pr[p];
                    }
                    ++q;
                }
            }
            run += all;
            at_run += at_all;
        }
        if (!EMIT && lane == 0) {
            A.above_count[c] = n_above;
            A.at_count[c] = n_at;
        }
    }
}

template <typename CodeT>
static int launch_top_hist(spk_ctx *ctx, int64_t n_chunks, unsigned long long *hist) {
    const int64_t P = ctx->n_pairs, n_pat = ctx->n_patterns;
    const bool lds = n_pat <= TOP_LDS_HIST;
    const int64_t cap = (lds ? SMP_WG_PER_CU : SEL_WG_PER_CU) * (int64_t)ctx->n_cu;  // LDS: fewer histograms to add up
    const int64_t g = std::max<int64_t>(std::min<int64_t>((n_chunks + SEL_WAVES - 1) / SEL_WAVES, cap), 1);
    const int64_t per_wg = ((n_chunks + g * SEL_WAVES - 1) / (g * SEL_WAVES)) * SEL_WAVES * SEL_CHUNK;
    SPK_REQUIRE(per_wg < ((int64_t)1 << 32), SPK_E_LIMIT, "spk_select_top: too many pairs");
    if (lds) k_top_hist<CodeT, true><<<(unsigned)g, SEL_THREADS, (size_t)n_pat * 4, ctx->stream>>>(ctx->codes.p, P, n_chunks, n_pat, hist);
    else k_top_hist<CodeT, false><<<(unsigned)g, SEL_THREADS, 0, ctx->stream>>>(ctx->codes.p, P, n_chunks, n_pat, hist);
    SPK_HIP(hipGetLastError());
    return SPK_OK;
}

template <typename CodeT, bool EMIT>
static int launch_top(spk_ctx *ctx, const TopArgs &A, bool lds) {
    const unsigned g = select_grid(ctx, A.n_chunks);
    if (lds) k_top<CodeT, true, EMIT><<<g, SEL_THREADS, (size_t)A.tab_words * 4, ctx->stream>>>(A);
    else k_top<CodeT, false, EMIT><<<g, SEL_THREADS, 0, ctx->stream>>>(A);
    SPK_HIP(hipGetLastError());
    return SPK_OK;
}

template <bool EMIT>
static int launch_top_codes(spk_ctx *ctx, const TopArgs &A, bool lds) {
    return ctx->code_bytes == 2 ? launch_top<uint16_t, EMIT>(ctx, A, lds) : launch_top<uint32_t, EMIT>(ctx, A, lds);
}

// What a top call found, for spk_select_top_info.
struct TopResult {
    int64_t eligible = 0, kept = 0, tied = 0, tied_kept = 0;
    double cut = __builtin_nan("");
    double ms = -1.0;
};

// The state after the picks, read back behind the scans: the at-the-cut pairs the emit pass keeps, and R's cut figures.
// at_total: the at-the-cut pairs the count pass found.
static int top_settle(int order, int64_t k, const unsigned long long *h_st, int64_t above_total, int64_t at_total,
                      TopResult &R, int64_t &r) {
    if (order == SPK_TOP_FIRST) {
        R.eligible = at_total;
        r = k;
    } else {
        R.eligible = (int64_t)h_st[TS_TOTAL];
        const int flag = (int)h_st[TS_FLAG];
        r = 0;
        if (flag == TOP_ACTIVE) {
            r = (int64_t)h_st[TS_REMAIN];
            R.tied = (int64_t)h_st[TS_TIED];
            R.tied_kept = r;
            R.cut = top_key_score(h_st[TS_PREFIX], order == SPK_TOP_DESC);
            SPK_REQUIRE(R.tied == at_total && r >= 1 && r <= R.tied, SPK_E_STATE, "spk_select_top: pairs at the cut");
        }
    }
    R.kept = above_total + std::min(at_total, r);
    SPK_REQUIRE(R.kept == std::min(k, R.eligible), SPK_E_STATE, "spk_select_top: kept count");
    return SPK_OK;
}

// spk_select_top's selection into S.  One host round trip, behind the scans.
static int build_top(spk_ctx *ctx, double lambda, double one_minus, const double *m, const double *u, int n_terms,
                     const spk_select_term *terms, int order, int64_t k, Selection &S, TopResult &R) {
    const int64_t P = ctx->n_pairs, n_pat = ctx->n_patterns;
    SelPatArgs PA{};
    PA.K = ctx->K;
    PA.n_pat = n_pat;
    for (int i = 0; i < ctx->K; ++i) {
        PA.stride[i] = (int32_t)ctx->stride[i];
        PA.nlev[i] = (uint8_t)ctx->n_levels[i];
    }
    for (int t = 0; t < n_terms; ++t) PA.terms[PA.n_terms++] = terms[t];
    selection_header(ctx, m && u, S);
    const bool scored = order != SPK_TOP_FIRST;
    StageTimer T{ctx};
    const int64_t words64 = (n_pat + 63) / 64, tab_bytes = (n_pat + 3) / 4 * 4;
    DevBuf<unsigned long long> keep, cnt, hist, st;
    DevBuf<uint8_t> tab, tmp, tmp_at;
    CountScan above, at;
    SPK_TRY(keep.alloc((size_t)words64 + 1));
    SPK_TRY(tab.alloc((size_t)tab_bytes + 4));
    SPK_TRY(st.alloc(TS_WORDS));
    SPK_TRY(hist.alloc(TOP_DIGITS));
    if (scored) SPK_TRY(cnt.alloc((size_t)n_pat + 1));
    if (S.has_mp) SPK_TRY(S.mpat.alloc((size_t)n_pat + 1));
    const int64_t n_chunks = (P + SEL_CHUNK - 1) / SEL_CHUNK;
    SPK_TRY(above.alloc(ctx, n_chunks));
    SPK_TRY(at.alloc(ctx, n_chunks));
    // ---- per pattern: mp table, keep bitset, pairs; the cut; the classes; per chunk: both counts; their scans
    const unsigned long long h_init[TS_WORDS] = {0ull, 0ull, (unsigned long long)(scored ? TOP_ACTIVE : TOP_FIRSTK), 0ull, 0ull};
    unsigned long long h_st[TS_WORDS] = {};  // read back behind the scans
    SPK_TRY(T.open());
    SPK_HIP(hipMemcpyAsync(st.p, h_init, sizeof(h_init), hipMemcpyHostToDevice, ctx->stream));
    SPK_HIP(hipMemsetAsync(tab.p, TOP_OUT, (size_t)tab_bytes + 4, ctx->stream));
    SPK_HIP(hipMemsetAsync(hist.p, 0, (size_t)TOP_DIGITS * 8, ctx->stream));
    if (S.has_mp) SPK_TRY(pattern_mp_table(ctx, lambda, one_minus, m, u, S.mpat.p));
    const unsigned pat_blocks = (unsigned)((n_pat + SEL_THREADS - 1) / SEL_THREADS);
    if (n_pat > 0) {
        k_select_patterns<<<pat_blocks, SEL_THREADS, 0, ctx->stream>>>(PA, S.mpat.p, keep.p);
        SPK_HIP(hipGetLastError());
    }
    if (scored) {
        SPK_HIP(hipMemsetAsync(cnt.p, 0, ((size_t)n_pat + 1) * 8, ctx->stream));
        if (n_chunks > 0) {
            if (ctx->code_bytes == 2) SPK_TRY(launch_top_hist<uint16_t>(ctx, n_chunks, cnt.p));
            else SPK_TRY(launch_top_hist<uint32_t>(ctx, n_chunks, cnt.p));
        }
        TopPatArgs H{};
        H.n_pat = n_pat;
        H.keep = keep.p;
        H.cnt = cnt.p;
        H.mpat = S.mpat.p;
        H.desc = order == SPK_TOP_DESC;
        H.hist = hist.p;
        H.st = st.p;
        const unsigned g = (unsigned)std::max<int64_t>(
            std::min<int64_t>(pat_blocks, TOP_PAT_WG_PER_CU * (int64_t)ctx->n_cu), 1);
        for (int pass = 0; pass < TOP_PASSES; ++pass) {
            H.pass = pass;
            k_top_pat_hist<<<g, SEL_THREADS, 0, ctx->stream>>>(H);
            SPK_HIP(hipGetLastError());
            k_top_pick<<<1, 64, 0, ctx->stream>>>(hist.p, st.p, k, pass);
            SPK_HIP(hipGetLastError());
        }
    }
    if (n_pat > 0) {
        k_top_classes<<<pat_blocks, SEL_THREADS, 0, ctx->stream>>>(n_pat, keep.p, S.mpat.p, order == SPK_TOP_DESC, st.p,
                                                                   tab.p);
        SPK_HIP(hipGetLastError());
    }
    TopArgs A{};
    A.codes = ctx->codes.p;
    A.P = P;
    A.n_chunks = n_chunks;
    A.tab = tab.p;
    A.n_pat = n_pat;
    A.tab_words = (int)(tab_bytes / 4);
    A.pl = S.has_rows ? ctx->pl.p : nullptr;
    A.pr = S.has_rows ? ctx->pr.p : nullptr;
    const bool lds = n_pat <= TOP_LDS_TAB;
    if (n_chunks > 0) {
        A.above_count = above.count.p;
        A.at_count = at.count.p;
        SPK_TRY(launch_top_codes<false>(ctx, A, lds));
    }
    SPK_TRY(exclusive_scan(ctx->stream, tmp_at, at.count.p, at.off.p, n_chunks + 1));
    SPK_HIP(hipMemcpyAsync(&at.total, at.off.p + n_chunks, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    SPK_HIP(hipMemcpyAsync(h_st, st.p, sizeof(h_st), hipMemcpyDeviceToHost, ctx->stream));
    SPK_TRY(scan_total(ctx, above, tmp, &T));  // synchronises
    int64_t r = 0;
    SPK_TRY(top_settle(order, k, h_st, above.total, at.total, R, r));
    const int64_t n_sel = R.kept;
    SPK_REQUIRE(n_sel >= 0 && n_sel <= P, SPK_E_STATE, "spk_select_top: survivor count");
    // ---- the survivors
    SPK_TRY(selection_alloc(S, n_sel));
    if (n_sel > 0) {
        A.above_count = A.at_count = nullptr;
        A.above_off = above.off.p;
        A.at_off = at.off.p;
        A.r = r;
        A.out_ord = S.ord.p;
        A.out_code = S.code.p;
        A.out_l = S.l.p;
        A.out_r = S.r.p;
        SPK_TRY(T.open());
        SPK_TRY(launch_top_codes<true>(ctx, A, lds));
        SPK_TRY(T.close());
    }
    S.n = n_sel;
    S.ms = R.ms = T.result();
    S.valid = true;
    return SPK_OK;
}

// ---- spk_select_top_of: the same over a selection's survivors ----
struct TopOfArgs {
    int64_t n, n_chunks;          // survivors, chunks of SEL_CHUNK
    const int64_t *ord;
    const int32_t *l, *r;         // or null (a selection without rows)
    const uint32_t *code;
    const double *mpat;           // SPK_SEL_MP: score = mpat[code] ...
    int64_t n_pat;
    const double *tf_mp;          // ... SPK_SEL_TF_MP: score = tf_mp[i]; both null: SPK_TOP_FIRST
    const double *cp_tf, *cp_adj; // emit pass: the selection's tf outputs to copy, or null
    int n_tf;
    int desc, pass;
    unsigned long long *hist;     // [TOP_DIGITS], zero at launch
    const unsigned long long *st;
    int64_t r_keep;               // emit pass: the at-the-cut survivors kept
    int64_t *above_count, *at_count;
    const int64_t *above_off, *at_off;
    int64_t *out_ord;
    int32_t *out_l, *out_r;
    uint32_t *out_code;
    double *out_tf, *out_adj;
};

// Survivor i < n's key.  A code outside the table (spk_select kept no such code) counts as NULL.
__device__ inline unsigned long long topof_key(const TopOfArgs &A, int64_t i) {
    double s = __builtin_nan("");
    if (A.tf_mp) {
        s = A.tf_mp[i];
    } else if (A.mpat) {
        const int64_t c = A.code[i];
        if (c < A.n_pat) s = A.mpat[c];
    }
    return top_key(s, A.desc != 0);
}

__global__ __launch_bounds__(SEL_THREADS) void k_topof_hist(TopOfArgs A) {
    __shared__ uint32_t s_h[TOP_DIGITS];
    if (A.pass > 0 && A.st[TS_FLAG] != (unsigned long long)TOP_ACTIVE) return;  // settled (grid-uniform)
    for (int i = threadIdx.x; i < TOP_DIGITS; i += SEL_THREADS) s_h[i] = 0u;
    __syncthreads();
    const unsigned long long prefix = A.pass > 0 ? A.st[TS_PREFIX] : 0ull;
    const int shift = 56 - 8 * A.pass;
    for (int64_t i = (int64_t)blockIdx.x * SEL_THREADS + threadIdx.x; i < A.n; i += (int64_t)gridDim.x * SEL_THREADS) {
        const unsigned long long key = topof_key(A, i);
        if (A.pass > 0 && (key >> (shift + 8)) != (prefix >> (shift + 8))) continue;
        atomicAdd(&s_h[(int)((key >> shift) & 255ull)], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < TOP_DIGITS; i += SEL_THREADS) {
        const uint32_t n = s_h[i];
        if (n) atomicAdd(&A.hist[i], (unsigned long long)n);
    }
}

// spk_select_best's chunk layout: one wave per chunk of SEL_CHUNK survivors, 64 consecutive survivors per slab.
template <bool EMIT>
__global__ __launch_bounds__(SEL_THREADS) void k_topof(TopOfArgs A) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int flag = (int)A.st[TS_FLAG];
    const unsigned long long cut = A.st[TS_PREFIX];
    const int64_t n_waves = (int64_t)gridDim.x * SEL_WAVES;
    for (int64_t c = (int64_t)blockIdx.x * SEL_WAVES + wave; c < A.n_chunks; c += n_waves) {
        int64_t run = 0, at_run = 0;
        if (EMIT) {
            at_run = A.at_off[c];
            run = A.above_off[c] + top_min(at_run, A.r_keep);
            if (A.above_off[c + 1] + top_min(A.at_off[c + 1], A.r_keep) == run) continue;  // wave-uniform
        }
        const int64_t base = c * SEL_CHUNK;
        int n_above = 0, n_at = 0;
        for (int s = 0; s < (int)(SEL_CHUNK / 64); ++s) {
            const int64_t i0 = base + (int64_t)s * 64;
            if (i0 >= A.n) break;  // wave-uniform
            const int64_t i = i0 + lane;
            int cls = TOP_OUT;
            if (i < A.n) cls = top_class(flag, cut, flag == TOP_ACTIVE ? topof_key(A, i) : 0ull);
            const unsigned long long wa = __ballot(cls == TOP_ABOVE), wt = __ballot(cls == TOP_AT);
            if (!EMIT) {
                n_above += __popcll(wa);
                n_at += __popcll(wt);
                continue;
            }
            const bool keep = cls == TOP_ABOVE || (cls == TOP_AT && at_run + __popcll(wt & below) < A.r_keep);
            const unsigned long long w = __ballot(keep);
            if (keep) {  // i < n
                const int64_t q = run + __popcll(w & below);
                A.out_ord[q] = A.ord[i];
                A.out_code[q] = A.code[i];
                if (A.l) {
                    A.out_l[q] = A.l[i];
                    A.out_r[q] = A.r[i];
                }
                if (A.out_tf) A.out_tf[q] = A.cp_tf[i];
                if (A.out_adj)
                    for (int t = 0; t < A.n_tf; ++t) A.out_adj[q * A.n_tf + t] = A.cp_adj[i * A.n_tf + t];
            }
            run += __popcll(w);
            at_run += __popcll(wt);
        }
        if (!EMIT && lane == 0) {
            A.above_count[c] = n_above;
            A.at_count[c] = n_at;
        }
    }
}

// The narrowing of S (the context's former selection, now a local of spk_select_top_of) into T.
static int narrow_top(spk_ctx *ctx, Selection &S, int field, int order, int64_t k, Selection &T, TopResult &R) {
    hipStream_t stream = ctx->stream;
    const int64_t n = S.n;
    T.K = S.K;
    T.n_levels = S.n_levels;
    T.stride = S.stride;
    T.has_rows = S.has_rows;
    T.has_mp = S.has_mp;
    T.has_tf = S.has_tf;
    T.n_tf = S.n_tf;
    T.pairs_epoch = S.pairs_epoch;
    T.gamma_seq = S.gamma_seq;
    T.fix_seq = S.fix_seq;
    T.ms = S.ms;  // spk_select_info keeps its meaning: the time of the selection's own kernels
    const bool scored = order != SPK_TOP_FIRST;
    StageTimer watch{ctx};
    const int64_t n_chunks = (n + SEL_CHUNK - 1) / SEL_CHUNK;
    TopOfArgs A{};
    DevBuf<unsigned long long> hist, st;
    DevBuf<uint8_t> tmp, tmp_at;
    CountScan above, at;
    const unsigned long long h_init[TS_WORDS] = {0ull, 0ull, (unsigned long long)(scored ? TOP_ACTIVE : TOP_FIRSTK), 0ull, 0ull};
    unsigned long long h_st[TS_WORDS] = {};  // read back behind the scans
    int64_t r = 0;
    if (n > 0) {
        SPK_TRY(hist.alloc(TOP_DIGITS));
        SPK_TRY(st.alloc(TS_WORDS));
        SPK_TRY(above.alloc(ctx, n_chunks));
        SPK_TRY(at.alloc(ctx, n_chunks));
        A.n = n;
        A.n_chunks = n_chunks;
        A.ord = S.ord.p;
        A.l = S.has_rows ? S.l.p : nullptr;
        A.r = S.has_rows ? S.r.p : nullptr;
        A.code = S.code.p;
        if (scored && field == SPK_SEL_MP) {
            A.mpat = S.mpat.p;
            A.n_pat = (int64_t)S.mpat.n - 1;  // the selecting calls allocate n_patterns + 1
        }
        if (scored && field == SPK_SEL_TF_MP) A.tf_mp = S.tf_mp.p;
        A.n_tf = S.n_tf;
        A.desc = order == SPK_TOP_DESC;
        A.hist = hist.p;
        A.st = st.p;
        A.above_count = above.count.p;
        A.at_count = at.count.p;
        const unsigned g = select_grid(ctx, n_chunks);
        SPK_REQUIRE(n < ((int64_t)1 << 32), SPK_E_LIMIT, "spk_select_top_of: too many survivors");  // k_topof_hist's counters
        SPK_TRY(watch.open());
        SPK_HIP(hipMemcpyAsync(st.p, h_init, sizeof(h_init), hipMemcpyHostToDevice, stream));
        SPK_HIP(hipMemsetAsync(hist.p, 0, (size_t)TOP_DIGITS * 8, stream));
        if (scored) {
            for (int pass = 0; pass < TOP_PASSES; ++pass) {
                A.pass = pass;
                k_topof_hist<<<g, SEL_THREADS, 0, stream>>>(A);
                SPK_HIP(hipGetLastError());
                k_top_pick<<<1, 64, 0, stream>>>(hist.p, st.p, k, pass);
                SPK_HIP(hipGetLastError());
            }
        }
        k_topof<false><<<g, SEL_THREADS, 0, stream>>>(A);
        SPK_HIP(hipGetLastError());
        SPK_TRY(exclusive_scan(stream, tmp_at, at.count.p, at.off.p, n_chunks + 1));
        SPK_HIP(hipMemcpyAsync(&at.total, at.off.p + n_chunks, sizeof(int64_t), hipMemcpyDeviceToHost, stream));
        SPK_HIP(hipMemcpyAsync(h_st, st.p, sizeof(h_st), hipMemcpyDeviceToHost, stream));
        SPK_TRY(scan_total(ctx, above, tmp, &watch));  // synchronises
        SPK_TRY(top_settle(order, k, h_st, above.total, at.total, R, r));
        SPK_REQUIRE(R.eligible == n, SPK_E_STATE, "spk_select_top_of: survivor count");
    }
    const int64_t kept = R.kept;
    SPK_TRY(T.ord.alloc((size_t)kept + 1));
    SPK_TRY(T.code.alloc((size_t)kept + 1));
    if (S.has_rows) {
        SPK_TRY(T.l.alloc((size_t)kept + 1));
        SPK_TRY(T.r.alloc((size_t)kept + 1));
    }
    if (S.has_tf) {
        SPK_TRY(T.tf_mp.alloc((size_t)kept + 1));
        SPK_TRY(T.adj.alloc((size_t)kept * S.n_tf + 1));
    }
    if (kept > 0) {
        A.above_count = A.at_count = nullptr;
        A.above_off = above.off.p;
        A.at_off = at.off.p;
        A.r_keep = r;
        A.out_ord = T.ord.p;
        A.out_l = T.l.p;
        A.out_r = T.r.p;
        A.out_code = T.code.p;
        if (S.has_tf) {
            A.cp_tf = S.tf_mp.p;
            A.cp_adj = S.adj.p;
            A.out_tf = T.tf_mp.p;
            A.out_adj = S.n_tf > 0 ? T.adj.p : nullptr;
        }
        SPK_TRY(watch.open());
        k_topof<true><<<select_grid(ctx, n_chunks), SEL_THREADS, 0, stream>>>(A);
        SPK_HIP(hipGetLastError());
        SPK_TRY(watch.close());
    }
    T.mpat = std::move(S.mpat);
    T.n = kept;
    T.valid = true;
    R.ms = watch.result();
    return SPK_OK;
}

}  // namespace spk

using namespace spk;

// What spk_select and spk_select_tf* check alike, after dropping the previous selection: the arguments first
// (SPK_E_INVALID), then the state.  tf: SPK_SEL_TF_MP terms are legal, m / u are required, and so is a pair set with
// rows.
static int select_begin(spk_ctx *ctx, const char *what, const double *m, const double *u, int n_terms,
                        const spk_select_term *terms, bool tf) {
    const std::string w(what);
    SPK_REQUIRE(ctx, SPK_E_INVALID, w + ": null ctx");
    SPK_HIP(hipSetDevice(ctx->device));
    ctx->sel.clear();  // whatever happens below, the previous selection is gone
    SPK_REQUIRE(n_terms >= 0 && n_terms <= SPK_SELECT_MAX_TERMS, SPK_E_INVALID,
                w + ": at most SPK_SELECT_MAX_TERMS (8) terms");
    SPK_REQUIRE(n_terms == 0 || terms, SPK_E_INVALID, w + ": null terms");
    SPK_REQUIRE((m == nullptr) == (u == nullptr), SPK_E_INVALID, w + ": m and u come together");
    SPK_REQUIRE(!tf || (m && u), SPK_E_INVALID, w + ": m and u are required");
    SPK_REQUIRE(ctx->codes_valid, SPK_E_STATE, w + ": no gammas");
    SPK_TRY(settle_gammas(ctx, nullptr));
    SPK_REQUIRE(ctx->codes_valid, SPK_E_STATE, w + ": no gammas");
    SPK_REQUIRE(ctx->K <= SEL_MAXK, SPK_E_LIMIT, w + ": too many comparison columns");
    for (int t = 0; t < n_terms; ++t) {
        const spk_select_term &T = terms[t];
        SPK_REQUIRE(T.field == SPK_SEL_MP || T.field == SPK_SEL_GAMMA || (tf && T.field == SPK_SEL_TF_MP), SPK_E_INVALID,
                    w + ": unknown field");
        SPK_REQUIRE(T.op >= SPK_SEL_LT && T.op <= SPK_SEL_IS_NOT_NULL, SPK_E_INVALID, w + ": unknown operator");
        SPK_REQUIRE(T.field != SPK_SEL_MP || (m && u), SPK_E_INVALID, w + ": a match_probability term needs m and u");
        SPK_REQUIRE(T.field != SPK_SEL_GAMMA || (T.col >= 0 && T.col < ctx->K), SPK_E_INVALID,
                    w + ": gamma column out of range");
    }
    if (tf) {
        const int64_t P = ctx->n_pairs;
        SPK_REQUIRE(ctx->pairs_valid && ctx->pl.p && ctx->pr.p && ctx->pl.n >= (size_t)P && ctx->pr.n >= (size_t)P,
                    SPK_E_STATE, w + ": no pair rows (a loaded gamma table)");
    }
    return SPK_OK;
}

extern "C" int spk_select(spk_ctx *ctx, double lambda, double one_minus, const double *m, const double *u,
                          int n_terms, const spk_select_term *terms, int64_t *out_n_selected) {
    SPK_TRY(select_begin(ctx, "spk_select", m, u, n_terms, terms, false));
    Selection S;
    SPK_TRY(build_selection(ctx, lambda, one_minus, m, u, n_terms, terms, nullptr, S));
    ctx->sel = std::move(S);
    if (out_n_selected) *out_n_selected = ctx->sel.n;
    return SPK_OK;
}

extern "C" int spk_select_tf(spk_ctx *ctx, double lambda, double one_minus, const double *m, const double *u,
                             int n_tf_cols, const int64_t *const *ids_side0, const int64_t *const *ids_side1,
                             const double *const *adj_tables, const int64_t *table_sizes, int n_terms,
                             const spk_select_term *terms, int64_t *out_n_selected) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "spk_select_tf: null ctx");
    SPK_HIP(hipSetDevice(ctx->device));
    ctx->sel.clear();  // a failing call leaves no selection
    SPK_REQUIRE(n_tf_cols >= 1 && n_tf_cols <= 8, SPK_E_INVALID, "spk_select_tf: 1..8 columns");
    SPK_REQUIRE(ids_side0 && ids_side1 && adj_tables && table_sizes, SPK_E_INVALID, "spk_select_tf: null arg");
    SPK_TRY(select_begin(ctx, "spk_select_tf", m, u, n_terms, terms, true));
    TfStage G;  // the id arrays and tables live until this call returns
    SPK_TRY(tf_stage_host_ids(ctx, n_tf_cols, ids_side0, ids_side1, G));
    SPK_TRY(tf_stage_tables(ctx, adj_tables, table_sizes, G));
    Selection S;
    SPK_TRY(build_selection(ctx, lambda, one_minus, m, u, n_terms, terms, &G.T, S));
    ctx->sel = std::move(S);
    if (out_n_selected) *out_n_selected = ctx->sel.n;
    return SPK_OK;
}

extern "C" int spk_select_tf_columns(spk_ctx *ctx, double lambda, double one_minus, const double *m, const double *u,
                                     int n_tf_cols, const int32_t *cols, const double *const *adj_tables,
                                     const int64_t *table_sizes, int n_terms, const spk_select_term *terms,
                                     int64_t *out_n_selected) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "spk_select_tf_columns: null ctx");
    SPK_HIP(hipSetDevice(ctx->device));
    ctx->sel.clear();  // a failing call leaves no selection
    SPK_REQUIRE(n_tf_cols >= 1 && n_tf_cols <= 8, SPK_E_INVALID, "spk_select_tf_columns: 1..8 columns");
    SPK_REQUIRE(cols && adj_tables && table_sizes, SPK_E_INVALID, "spk_select_tf_columns: null arg");
    SPK_TRY(select_begin(ctx, "spk_select_tf_columns", m, u, n_terms, terms, true));
    TfStage G;
    SPK_TRY(tf_stage_column_ids(ctx, n_tf_cols, cols, G));
    SPK_TRY(tf_stage_tables(ctx, adj_tables, table_sizes, G));
    Selection S;
    SPK_TRY(build_selection(ctx, lambda, one_minus, m, u, n_terms, terms, &G.T, S));
    ctx->sel = std::move(S);
    if (out_n_selected) *out_n_selected = ctx->sel.n;
    return SPK_OK;
}

extern "C" int spk_select_sample(spk_ctx *ctx, double lambda, double one_minus, const double *m, const double *u,
                                 int n_terms, const spk_select_term *terms, int n_strata, const double *edges,
                                 const int64_t *quota, uint64_t seed, int64_t *out_n_selected) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "spk_select_sample: null ctx");
    SPK_HIP(hipSetDevice(ctx->device));
    ctx->sel.clear();  // a failing call leaves no selection, and no figures for spk_select_sample_info
    ctx->strata_pop.clear();
    ctx->strata_kept.clear();
    ctx->strata_ms = -1.0;
    SPK_REQUIRE(n_strata >= 1 && n_strata <= SPK_SAMPLE_MAX_STRATA, SPK_E_INVALID,
                "spk_select_sample: 1..SPK_SAMPLE_MAX_STRATA (64) strata");
    SPK_REQUIRE(edges && quota, SPK_E_INVALID, "spk_select_sample: null arg");
    for (int b = 0; b <= n_strata; ++b) {
        SPK_REQUIRE(std::isfinite(edges[b]), SPK_E_INVALID, "spk_select_sample: an edge is not finite");
        SPK_REQUIRE(b == 0 || edges[b - 1] < edges[b], SPK_E_INVALID, "spk_select_sample: edges not strictly ascending");
    }
    for (int b = 0; b < n_strata; ++b) SPK_REQUIRE(quota[b] >= 0, SPK_E_INVALID, "spk_select_sample: negative quota");
    SPK_REQUIRE(m && u, SPK_E_INVALID, "spk_select_sample: m and u are required");
    SPK_TRY(select_begin(ctx, "spk_select_sample", m, u, n_terms, terms, false));
    Selection S;
    std::vector<int64_t> pop, kept;
    SPK_TRY(build_sample(ctx, lambda, one_minus, m, u, n_terms, terms, n_strata, edges, quota, seed, S, pop, kept));
    ctx->sel = std::move(S);
    ctx->strata_pop = std::move(pop);
    ctx->strata_kept = std::move(kept);
    ctx->strata_ms = ctx->sel.ms;
    if (out_n_selected) *out_n_selected = ctx->sel.n;
    return SPK_OK;
}

extern "C" int spk_select_sample_info(spk_ctx *ctx, int *out_n_strata, int64_t *out_population, int64_t *out_kept,
                                      double *out_ms) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "spk_select_sample_info: null ctx");
    const size_t n = ctx->strata_pop.size();
    if (out_n_strata) *out_n_strata = n ? (int)n : -1;
    if (out_population) std::copy(ctx->strata_pop.begin(), ctx->strata_pop.end(), out_population);
    if (out_kept) std::copy(ctx->strata_kept.begin(), ctx->strata_kept.end(), out_kept);
    if (out_ms) *out_ms = n ? ctx->strata_ms : -1.0;
    return SPK_OK;
}

// A top call starts without figures (a failing one leaves none) and ends by recording them.
static void top_info_clear(spk_ctx *ctx) {
    ctx->top_eligible = ctx->top_kept = ctx->top_tied = ctx->top_tied_kept = -1;
    ctx->top_cut = __builtin_nan("");
    ctx->top_ms = -1.0;
}

static void top_info_set(spk_ctx *ctx, const TopResult &R) {
    ctx->top_eligible = R.eligible;
    ctx->top_kept = R.kept;
    ctx->top_tied = R.tied;
    ctx->top_tied_kept = R.tied_kept;
    ctx->top_cut = R.cut;
    ctx->top_ms = R.ms;
}

extern "C" int spk_select_top(spk_ctx *ctx, double lambda, double one_minus, const double *m, const double *u,
                              int n_terms, const spk_select_term *terms, int order, int64_t k, int64_t *out_n_selected) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "spk_select_top: null ctx");
    SPK_HIP(hipSetDevice(ctx->device));
    ctx->sel.clear();  // a failing call leaves no selection, and no figures for spk_select_top_info
    top_info_clear(ctx);
    SPK_REQUIRE(order >= SPK_TOP_FIRST && order <= SPK_TOP_DESC, SPK_E_INVALID,
                "spk_select_top: unknown order (SPK_TOP_FIRST, _ASC or _DESC)");
    SPK_REQUIRE(k >= 0, SPK_E_INVALID, "spk_select_top: negative k");
    SPK_REQUIRE(order == SPK_TOP_FIRST || (m && u), SPK_E_INVALID, "spk_select_top: a score order needs m and u");
    SPK_TRY(select_begin(ctx, "spk_select_top", m, u, n_terms, terms, false));
    Selection S;
    TopResult R;
    SPK_TRY(build_top(ctx, lambda, one_minus, m, u, n_terms, terms, order, k, S, R));
    ctx->sel = std::move(S);
    top_info_set(ctx, R);
    if (out_n_selected) *out_n_selected = ctx->sel.n;
    return SPK_OK;
}

extern "C" int spk_select_top_of(spk_ctx *ctx, int field, int order, int64_t k, int64_t *out_n_kept) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "spk_select_top_of: null ctx");
    SPK_HIP(hipSetDevice(ctx->device));
    Selection S = std::move(ctx->sel);  // freed when this call returns, whatever happens below ...
    ctx->sel.clear();                   // ... and a failing call leaves no selection
    top_info_clear(ctx);
    SPK_REQUIRE(order >= SPK_TOP_FIRST && order <= SPK_TOP_DESC, SPK_E_INVALID,
                "spk_select_top_of: unknown order (SPK_TOP_FIRST, _ASC or _DESC)");
    SPK_REQUIRE(order == SPK_TOP_FIRST || field == SPK_SEL_MP || field == SPK_SEL_TF_MP, SPK_E_INVALID,
                "spk_select_top_of: unknown field (SPK_SEL_MP or SPK_SEL_TF_MP)");
    SPK_REQUIRE(k >= 0, SPK_E_INVALID, "spk_select_top_of: negative k");
    SPK_REQUIRE(S.valid, SPK_E_STATE, "spk_select_top_of: no selection (run spk_select)");
    SPK_REQUIRE(S.current(ctx), SPK_E_STATE, "spk_select_top_of: the pairs or codes changed since spk_select");
    if (order != SPK_TOP_FIRST) {
        SPK_REQUIRE(field != SPK_SEL_MP || S.has_mp, SPK_E_STATE,
                    "spk_select_top_of: no match_probability (spk_select got no m / u)");
        SPK_REQUIRE(field != SPK_SEL_TF_MP || S.has_tf, SPK_E_STATE,
                    "spk_select_top_of: no tf_adjusted_match_prob (the selection was made without tf tables, spk_select)");
    }
    Selection T;
    TopResult R;
    SPK_TRY(narrow_top(ctx, S, field, order, k, T, R));
    ctx->sel = std::move(T);
    top_info_set(ctx, R);
    if (out_n_kept) *out_n_kept = ctx->sel.n;
    return SPK_OK;
}

extern "C" int spk_select_top_info(spk_ctx *ctx, int64_t *out_eligible, int64_t *out_kept, double *out_cut_score,
                                   int64_t *out_tied, int64_t *out_tied_kept, double *out_ms) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "spk_select_top_info: null ctx");
    if (out_eligible) *out_eligible = ctx->top_eligible;
    if (out_kept) *out_kept = ctx->top_kept;
    if (out_cut_score) *out_cut_score = ctx->top_cut;
    if (out_tied) *out_tied = ctx->top_tied;
    if (out_tied_kept) *out_tied_kept = ctx->top_tied_kept;
    if (out_ms) *out_ms = ctx->top_ms;
    return SPK_OK;
}

extern "C" int spk_select_copy_tf(spk_ctx *ctx, int64_t start, int64_t count, double *out_tf_mp, double *out_adj) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "spk_select_copy_tf: null ctx");
    const Selection &S = ctx->sel;
    SPK_REQUIRE(S.valid, SPK_E_STATE, "spk_select_copy_tf: no selection (run spk_select_tf*)");
    SPK_REQUIRE(S.has_tf, SPK_E_STATE, "spk_select_copy_tf: the selection was made without tf tables (spk_select)");
    SPK_REQUIRE(S.current(ctx), SPK_E_STATE, "spk_select_copy_tf: the pairs or codes changed since spk_select_tf*");
    SPK_REQUIRE(start >= 0 && count >= 0 && start + count <= S.n, SPK_E_INVALID, "spk_select_copy_tf: range");
    if (!count) return SPK_OK;
    SPK_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (out_tf_mp) SPK_HIP(hipMemcpyAsync(out_tf_mp, S.tf_mp.p + start, (size_t)count * 8, hipMemcpyDeviceToHost, st));
    if (out_adj)
        SPK_HIP(hipMemcpyAsync(out_adj, S.adj.p + start * S.n_tf, (size_t)count * S.n_tf * 8, hipMemcpyDeviceToHost, st));
    SPK_HIP(hipStreamSynchronize(st));
    return SPK_OK;
}

extern "C" int spk_select_copy(spk_ctx *ctx, int64_t start, int64_t count, int64_t *out_ordinal, int32_t *out_l,
                               int32_t *out_r, int8_t *out_gammas, double *out_mp) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "spk_select_copy: null ctx");
    const Selection &S = ctx->sel;
    SPK_REQUIRE(S.valid, SPK_E_STATE, "spk_select_copy: no selection (run spk_select)");
    SPK_REQUIRE(S.current(ctx), SPK_E_STATE, "spk_select_copy: the pairs or codes changed since spk_select");
    SPK_REQUIRE(start >= 0 && count >= 0 && start + count <= S.n, SPK_E_INVALID, "spk_select_copy: range");
    SPK_REQUIRE(!(out_l || out_r) || S.has_rows, SPK_E_STATE, "spk_select_copy: no pair rows (a loaded gamma table)");
    SPK_REQUIRE(!out_mp || S.has_mp, SPK_E_STATE, "spk_select_copy: spk_select got no m / u");
    if (!count) return SPK_OK;
    SPK_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (out_ordinal) SPK_HIP(hipMemcpyAsync(out_ordinal, S.ord.p + start, (size_t)count * 8, hipMemcpyDeviceToHost, st));
    if (out_l) SPK_HIP(hipMemcpyAsync(out_l, S.l.p + start, (size_t)count * 4, hipMemcpyDeviceToHost, st));
    if (out_r) SPK_HIP(hipMemcpyAsync(out_r, S.r.p + start, (size_t)count * 4, hipMemcpyDeviceToHost, st));
    DevBuf<int8_t> d_g;
    DevBuf<double> d_mp;
    if (out_gammas || out_mp) {
        SelDecodeArgs D{};
        D.start = start;
        D.count = count;
        D.K = S.K;
        D.code = S.code.p;
        D.mpat = S.mpat.p;
        for (int k = 0; k < S.K; ++k) {
            D.stride[k] = (int32_t)S.stride[k];
            D.nlev[k] = (uint8_t)S.n_levels[k];
        }
        if (out_gammas && S.K > 0) {
            SPK_TRY(d_g.alloc((size_t)count * S.K));
            D.out_g = d_g.p;
        }
        if (out_mp) {
            SPK_TRY(d_mp.alloc((size_t)count));
            D.out_mp = d_mp.p;
        }
        k_select_decode<<<(unsigned)((count + 255) / 256), 256, 0, st>>>(D);
        SPK_HIP(hipGetLastError());
        if (D.out_g) SPK_HIP(hipMemcpyAsync(out_gammas, d_g.p, (size_t)count * S.K, hipMemcpyDeviceToHost, st));
        if (D.out_mp) SPK_HIP(hipMemcpyAsync(out_mp, d_mp.p, (size_t)count * 8, hipMemcpyDeviceToHost, st));
    }
    SPK_HIP(hipStreamSynchronize(st));
    return SPK_OK;
}

extern "C" int spk_select_info(spk_ctx *ctx, int64_t *out_n_selected, double *out_ms) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "spk_select_info: null ctx");
    if (out_n_selected) *out_n_selected = ctx->sel.valid ? ctx->sel.n : -1;
    if (out_ms) *out_ms = ctx->sel.valid ? ctx->sel.ms : -1.0;
    return SPK_OK;
}

extern "C" int spk_select_release(spk_ctx *ctx) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "spk_select_release: null ctx");
    SPK_HIP(hipSetDevice(ctx->device));
    SPK_HIP(hipStreamSynchronize(ctx->stream));
    ctx->sel.clear();
    return SPK_OK;
}
