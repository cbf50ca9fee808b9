// Pairs against labels (no counterpart in the reference release; later releases: truth_space_table_from_labels_column,
// estimate_m_from_label_column).  One pass over the pairs counts them per (truth state, comparison pattern):
// state = NON_MATCH / MATCH / UNKNOWN from the two records' label ids, pattern = the pair's packed code.  Since
// match_probability is a function of the pattern alone (pattern_mp, spk_em.hip), these 3 x n_patterns integers give
// the host the exact confusion matrix at every threshold, the pairs blocking never produced and the supervised
// m / u / lambda estimate, without one pair leaving the device.  The counts are integers: order-free, identical for
// any grid, and they sum exactly over the ranks of a sharded job, as the EM histogram does.
//
// Layout: state-major, counts[s * n_patterns + code].  Each state's row is then an n_patterns vector in the EM
// histogram's own order (the three rows sum to it bin for bin), and the host slices rows instead of striding.
#include <algorithm>
#include <cstring>

#include "spk_internal.h"
#include "spk_tf_pair.h"

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "spk_labels.hip targets gfx950 (MI355X) only"
#endif

namespace spk {

// How a wave adds its keys (a compile-time switch for tools/ab_labels.py's A/B; same counts in every form):
// 0 (default) = the LDS variant without aggregation, one LDS atomic per pair, and the global variant with ballot
// aggregation (the leader's key by shuffle); 1 = ballot aggregation in both variants; 2 = as 1 with the leader's key
// read by v_readlane.  cfg2 (576 patterns, LDS variant), device ms of the call: 0.191 / 0.231 / 0.252
// (profiles/ab_labels_agg.log): the ballot rounds cost more than the same-address LDS atomics they save.
#ifndef SPK_LABEL_AGG
#define SPK_LABEL_AGG 0
#endif

constexpr int LH_THREADS = 512;
constexpr int LH_PAIRS = 8;              // pairs per lane and step: two 16-byte vectors of each side's rows
constexpr int LH_LDS_BYTES = 64 * 1024;  // LDS-privatised counters up to this (and the device attribute): two
                                         // workgroups of a CU's 160 KiB stay resident at the largest pattern space
constexpr int LH_WG_PER_CU = 4;          // 32 waves per CU while the counters are small: the gathers are latency
constexpr int64_t LH_BLOCK_PAIRS_MAX = (int64_t)1 << 31;  // pairs one workgroup may count (see label_grid)

// One label id per record, 64 -> 32 bits: negative = NULL = -1.  An id of 2^31 or more sets *bad.
__global__ void k_label_narrow(int64_t n, const int64_t *__restrict__ in, int32_t *__restrict__ out,
                               unsigned int *__restrict__ bad) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t v = in[i];
    if (v > (int64_t)INT32_MAX) *bad = 1u;
    out[i] = v < 0 ? -1 : (int32_t)v;
}

struct LabelArgs {
    int64_t P;
    const int32_t *pl, *pr;
    const int32_t *lab0, *lab1;  // label id per device row of the pairs' left / right table (-1 = NULL)
    uint32_t n0, n1;             // their row counts
    uint32_t n_pat;
    unsigned long long *ghist;   // [3 x n_pat], zeroed before the launch
    unsigned int *bad;           // set to 2 when a pair names a row or a code out of range (it is not counted)
};

// bin of one pair, or in = false when it names a row outside its table or a code outside the pattern space
__device__ __forceinline__ uint32_t label_bin(const LabelArgs &A, uint32_t l, uint32_t r, uint32_t c, bool &in) {
    if (in && (l >= A.n0 || r >= A.n1 || c >= A.n_pat)) {
        *A.bad = 2u;
        in = false;
    }
    if (!in) return 0xFFFFFFFFu;
    const int32_t a = A.lab0[l], b = A.lab1[r];  // the two gathers
    const uint32_t state = (a < 0 || b < 0) ? (uint32_t)SPK_LABEL_UNKNOWN : (uint32_t)(a == b);
    return state * A.n_pat + c;
}

// One step of a wave: every lane brings one key (in = false: none).  LDS: one LDS atomic per pair (SPK_LABEL_AGG 1, 2:
// up to four distinct keys of the wave are added once each by their first lane, the rest by plain LDS atomics,
// k_hist's form).  Global: one 64-bit add per distinct key of the wave, whatever their number (k_tf_hist's form).
// Every lane of the wave must call it.
template <bool LDS>
__device__ __forceinline__ void label_add(uint32_t key, bool in, int lane, uint32_t *sh,
                                          unsigned long long *__restrict__ ghist) {
    unsigned long long todo = __ballot(in);
#if SPK_LABEL_AGG == 0
    if (LDS) {  // no aggregation: every lane its own LDS atomic
        if (in) atomicAdd(&sh[key], 1u);
        return;
    }
#endif
    for (int it = 0; (!LDS || it < 4) && todo; ++it) {  // wave-uniform
        const int leader = __ffsll(todo) - 1;
#if SPK_LABEL_AGG != 2
        const uint32_t k = __shfl(key, leader);
#else
        const uint32_t k = (uint32_t)__builtin_amdgcn_readlane((int)key, leader);  // leader is wave-uniform
#endif
        const unsigned long long same = __ballot(in && key == k) & todo;
        if (lane == leader) {
            if (LDS) atomicAdd(&sh[k], (uint32_t)__popcll(same));
            else atomicAdd(&ghist[k], (unsigned long long)__popcll(same));
        }
        todo &= ~same;
    }
    if (LDS && ((todo >> lane) & 1ull)) atomicAdd(&sh[key], 1u);
}

// The label histogram.  Each lane takes LH_PAIRS consecutive pairs per step: their rows as two 16-byte vectors per
// side, their codes as one (uint16_t) or two (uint32_t) 16-byte vectors, all coalesced; then 16 independent label
// gathers (the 4-byte ids of up to a few million records: L2 / Infinity Cache resident), then the counts.
// LDS = true: 3 x n_pat 32-bit counters in the workgroup's LDS, flushed with 64-bit global atomics (an empty counter
// is not flushed).  A workgroup counts at most LH_BLOCK_PAIRS_MAX + LH_THREADS x LH_PAIRS < 2^32 pairs in all
// (label_grid), so no LDS word can wrap.  LDS = false: ballot-aggregated 64-bit global atomics.
template <typename CodeT, bool LDS>
__global__ __launch_bounds__(LH_THREADS) void k_label_hist(LabelArgs A, const CodeT *__restrict__ codes) {
    extern __shared__ uint32_t sh[];
    const int n_bins = 3 * (int)A.n_pat;
    if (LDS) {
        for (int b = threadIdx.x; b < n_bins; b += LH_THREADS) sh[b] = 0;
        __syncthreads();
    }
    const int lane = threadIdx.x & 63;
    const int64_t n_vec = A.P / LH_PAIRS;
    const uint4 *lv = reinterpret_cast<const uint4 *>(A.pl);
    const uint4 *rv = reinterpret_cast<const uint4 *>(A.pr);
    const uint4 *cv = reinterpret_cast<const uint4 *>(codes);
    constexpr int CW = LH_PAIRS * (int)sizeof(CodeT) / 16;  // 16-byte code vectors per step: 1 or 2
    for (int64_t v = (int64_t)blockIdx.x * LH_THREADS + threadIdx.x;; v += (int64_t)gridDim.x * LH_THREADS) {
        // wave-uniform loop exit keeps every lane inside the ballots of label_add
        bool in = v < n_vec;
        if (!__any(in)) break;
        uint32_t l[LH_PAIRS], r[LH_PAIRS], c[LH_PAIRS], key[LH_PAIRS];
        bool ok[LH_PAIRS];
        if (in) {
            const uint4 l0 = lv[2 * v], l1 = lv[2 * v + 1], r0 = rv[2 * v], r1 = rv[2 * v + 1];
            l[0] = l0.x, l[1] = l0.y, l[2] = l0.z, l[3] = l0.w, l[4] = l1.x, l[5] = l1.y, l[6] = l1.z, l[7] = l1.w;
            r[0] = r0.x, r[1] = r0.y, r[2] = r0.z, r[3] = r0.w, r[4] = r1.x, r[5] = r1.y, r[6] = r1.z, r[7] = r1.w;
            uint4 w[CW];
#pragma unroll
            for (int j = 0; j < CW; ++j) w[j] = cv[CW * v + j];
            const CodeT *e = reinterpret_cast<const CodeT *>(w);
#pragma unroll
            for (int j = 0; j < LH_PAIRS; ++j) c[j] = (uint32_t)e[j];
        }
#pragma unroll
        for (int j = 0; j < LH_PAIRS; ++j) {  // all the gathers first, so that they are in flight together
            ok[j] = in;
            key[j] = label_bin(A, in ? l[j] : 0u, in ? r[j] : 0u, in ? c[j] : 0u, ok[j]);
        }
#pragma unroll
        for (int j = 0; j < LH_PAIRS; ++j) label_add<LDS>(key[j], ok[j], lane, sh, A.ghist);
    }
    // tail (P not a multiple of LH_PAIRS): workgroup 0's first wave, one pair per lane, every lane in the ballots
    if (blockIdx.x == 0 && threadIdx.x < 64) {
        const int64_t p = n_vec * LH_PAIRS + lane;
        bool in = p < A.P;
        const uint32_t key = label_bin(A, in ? (uint32_t)A.pl[p] : 0u, in ? (uint32_t)A.pr[p] : 0u,
                                       in ? (uint32_t)codes[p] : 0u, in);
        label_add<LDS>(key, in, lane, sh, A.ghist);
    }
    if (LDS) {
        __syncthreads();
        for (int b = threadIdx.x; b < n_bins; b += LH_THREADS) {
            const uint32_t n = sh[b];
            if (n) atomicAdd(&A.ghist[b], (unsigned long long)n);
        }
    }
}

// Workgroups of the launch: enough for LH_WG_PER_CU per CU, never more than the steps there are, and never so few
// that one workgroup would count more than LH_BLOCK_PAIRS_MAX pairs (its LDS counters are 32-bit).
static unsigned label_grid(const spk_ctx *ctx, int64_t P, int wg_per_cu = LH_WG_PER_CU) {
    const int64_t steps = (P / LH_PAIRS + LH_THREADS - 1) / LH_THREADS;
    int64_t g = std::min<int64_t>(steps, wg_per_cu * (int64_t)ctx->n_cu);
    g = std::max<int64_t>(g, (P + LH_BLOCK_PAIRS_MAX - 1) / LH_BLOCK_PAIRS_MAX);
    return (unsigned)std::max<int64_t>(g, 1);
}

template <typename CodeT>
static int launch_label_hist(spk_ctx *ctx, const LabelArgs &A, bool lds) {
    const unsigned g = label_grid(ctx, A.P);
    const CodeT *codes = reinterpret_cast<const CodeT *>(ctx->codes.p);
    if (lds) k_label_hist<CodeT, true><<<g, LH_THREADS, (size_t)3 * A.n_pat * 4, ctx->stream>>>(A, codes);
    else k_label_hist<CodeT, false><<<g, LH_THREADS, 0, ctx->stream>>>(A, codes);
    SPK_HIP(hipGetLastError());
    return SPK_OK;
}

// The label ids of one call on the device, 32 bits per record in device row order: locals of the entry points.
struct LabelIds {
    DevBuf<int64_t> wide;
    DevBuf<int32_t> lab0, lab1;
    DevBuf<unsigned int> bad;  // [1]: 1 = an id of 2^31 or more (read here), 2 = set by the counting kernels
    bool second = false;       // the right rows have an id array of their own
    const int32_t *side0() const { return lab0.p; }
    const int32_t *side1() const { return second ? lab1.p : lab0.p; }
};

// Uploads and narrows the ids of n0 / n1 records (k_label_narrow, inside T's intervals; the upload itself is not a
// launch: outside them).  An id of 2^31 or more is SPK_E_INVALID.  Leaves *L.bad = 0 and the stream synchronised.
static int stage_label_ids(spk_ctx *ctx, const char *what, const int64_t *ids_side0, const int64_t *ids_side1,
                           int64_t n0, int64_t n1, StageTimer &T, LabelIds &L) {
    hipStream_t st = ctx->stream;
    L.second = ids_side1 && (ctx->link_type == SPK_LINK_ONLY || ids_side1 != ids_side0);
    SPK_TRY(L.wide.alloc((size_t)std::max(n0, L.second ? n1 : 0) + 1));
    SPK_TRY(L.lab0.alloc((size_t)n0 + 1));
    if (L.second) SPK_TRY(L.lab1.alloc((size_t)n1 + 1));
    SPK_TRY(L.bad.alloc(1));
    SPK_HIP(hipMemsetAsync(L.bad.p, 0, sizeof(unsigned int), st));
    auto narrow = [&](const int64_t *ids, int64_t n, int32_t *out) -> int {
        if (n == 0) return SPK_OK;
        SPK_HIP(hipMemcpyAsync(L.wide.p, ids, (size_t)n * 8, hipMemcpyHostToDevice, st));
        SPK_TRY(T.open());
        k_label_narrow<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(n, L.wide.p, out, L.bad.p);
        SPK_HIP(hipGetLastError());
        return T.close();  // synchronises: the next upload reuses `wide`; the source is borrowed for the call
    };
    SPK_TRY(narrow(ids_side0, n0, L.lab0.p));
    if (L.second) SPK_TRY(narrow(ids_side1, n1, L.lab1.p));
    unsigned int h_bad = 0u;
    SPK_HIP(hipMemcpyAsync(&h_bad, L.bad.p, sizeof(h_bad), hipMemcpyDeviceToHost, st));
    SPK_HIP(hipStreamSynchronize(st));
    SPK_REQUIRE(h_bad == 0u, SPK_E_INVALID, std::string(what) + ": a label id of 2^31 or more");
    return SPK_OK;
}

// ---- pairs per (truth state, score bin), the score decided per pair -------------------------------------------
// spk_label_scores_*: the counting that k_label_hist does per pattern, for scores that are not a function of the
// pattern alone (tf_adjusted_match_prob) or for pair sets that are not the context's (a selection's survivors).
// Thresholds t[0..T) ascending; bin(s) = #{k : s > t[k]} in 0..T (filter's `>`), a NaN score in bin T + 1; counters
// [3 x (T + 2)], state-major.  Both kernels keep the thresholds (8 T bytes) and 32-bit counters (12 (T + 2) bytes) in
// LDS -- 20.3 KB at T = 1024, so several workgroups stay resident per CU -- add with one LDS atomic per pair (no ballot
// aggregation: profiles/ab_labels_agg.log) and flush the non-empty counters with 64-bit global atomics.
constexpr int LS_THREADS = 256;
constexpr int LS_PAIRS = 8;       // all-pairs kernel: pairs per lane and step, as k_select_tf_count's slab (no scratch)
// Workgroups per CU the grid is capped at (a compile-time switch for tools/ab_label_scores.py's A/B): 3 is what
// k_label_scores_tf's 140 VGPRs keep resident (3 waves per SIMD, a workgroup puts one on each), so every workgroup
// runs from the first cycle and takes an equal share of the steps.  cfg2 link job, device ms of the call at T = 72 /
// 1024: 0.25 / 0.31 with 3, 0.32 / 0.40 with 4 (a quarter of the workgroups start when the others are done):
// profiles/ab_label_scores.log.
#ifndef SPK_LABEL_SCORE_WG_PER_CU
#define SPK_LABEL_SCORE_WG_PER_CU 3
#endif
constexpr int LS_WG_PER_CU = SPK_LABEL_SCORE_WG_PER_CU;
constexpr int LS_SEL_WG_PER_CU = 8;  // k_label_scores_sel (16 VGPRs): 32 waves per CU
constexpr int64_t LS_BLOCK_PAIRS_MAX = (int64_t)1 << 31;  // pairs one workgroup may count (32-bit LDS counters)

struct ScoreArgs {
    int64_t P;                   // pairs of the context, or survivors of the selection
    const int32_t *pl, *pr;      // their rows
    const int32_t *lab0, *lab1;  // label id per device row of the left / right table (-1 = NULL)
    uint32_t n0, n1;             // their row counts
    uint32_t n_pat;
    int T;                       // thresholds, 0..SPK_LABEL_SCORE_MAX_THRESHOLDS
    int top;                     // the largest power of two <= T (0: T = 0): the search's first stride
    const double *thr;           // [T] ascending, no NaN
    const double *mpat;          // mp per pattern [n_pat] (the call's own or the selection's), or null
    const uint32_t *code;        // selection kernel: the survivors' codes
    const double *per_pair;      // selection kernel: the survivors' tf_adjusted_match_prob, or null = mpat[code]
    unsigned long long *gcnt;    // [3 x (T + 2)], zeroed before the launch
    unsigned int *bad;           // set to 2 when a pair names a row or a code out of range (it is not counted)
};

// bin(s): the thresholds below s, by strides top, top / 2, .., 1 (at most 11, the same for every lane); the index is
// clamped so that every read lies inside th[0..T), and no step branches.
__device__ __forceinline__ uint32_t score_bin(double s, const double *th, uint32_t T, int top) {
    uint32_t pos = 0;
    for (int step = top; step > 0; step >>= 1) {
        const uint32_t k = pos + (uint32_t)step;  // >= 1
        const double t = th[min(k, T) - 1u];
        pos = (k <= T && s > t) ? k : pos;
    }
    return s != s ? T + 1u : pos;
}

__device__ __forceinline__ void score_add(uint32_t *cnt, const ScoreArgs &A, const double *th, int32_t a, int32_t b,
                                          double s) {
    const uint32_t state = (a < 0 || b < 0) ? (uint32_t)SPK_LABEL_UNKNOWN : (uint32_t)(a == b);
    atomicAdd(&cnt[state * ((uint32_t)A.T + 2u) + score_bin(s, th, (uint32_t)A.T, A.top)], 1u);
}

// LDS of both kernels: the thresholds, then the counters (cleared); ends with a barrier.
__device__ __forceinline__ uint32_t *score_lds_init(const ScoreArgs &A, double *s_th) {
    uint32_t *cnt = reinterpret_cast<uint32_t *>(s_th + A.T);
    for (int i = threadIdx.x; i < A.T; i += LS_THREADS) s_th[i] = A.thr[i];
    for (int b = threadIdx.x; b < 3 * (A.T + 2); b += LS_THREADS) cnt[b] = 0;
    __syncthreads();
    return cnt;
}

__device__ __forceinline__ void score_lds_flush(const ScoreArgs &A, const uint32_t *cnt) {
    __syncthreads();
    for (int b = threadIdx.x; b < 3 * (A.T + 2); b += LS_THREADS) {
        const uint32_t n = cnt[b];
        if (n) atomicAdd(&A.gcnt[b], (unsigned long long)n);
    }
}

// Every pair of the context against the labels, by tf_adjusted_match_prob under the call's tables F and mp table.
// k_label_hist's shape: each lane takes LS_PAIRS consecutive pairs per step, their rows as two 16-byte vectors per
// side and their codes as one (uint16_t) or two (uint32_t), all coalesced; the loop exit is wave-uniform; the tail
// (P mod LS_PAIRS) is workgroup 0's first wave.  The gathers are issued as k_select_tf_count issues them: the labels
// and mp of all the lane's pairs, then column by column the value ids of every pair, the table entries, the fold
// (tf_begin / tf_adj / tf_fold / tf_finish, spk_tf_pair.h: the bits of spk_tf_apply*).  A row or a code out of range
// sets *bad and the pair gathers and counts nothing.  A workgroup counts at most LS_BLOCK_PAIRS_MAX + one step's
// pairs (score_grid), so no LDS word wraps.
template <typename CodeT>
__global__ __launch_bounds__(LS_THREADS) void k_label_scores_tf(ScoreArgs A, TfApply F, const CodeT *__restrict__ codes) {
    extern __shared__ __attribute__((aligned(16))) double s_th[];
    uint32_t *cnt = score_lds_init(A, s_th);
    constexpr int V = LS_PAIRS;
    const int lane = threadIdx.x & 63;
    const int64_t n_vec = A.P / V;
    const uint4 *lv = reinterpret_cast<const uint4 *>(A.pl);
    const uint4 *rv = reinterpret_cast<const uint4 *>(A.pr);
    const uint4 *cv = reinterpret_cast<const uint4 *>(codes);
    constexpr int CW = V * (int)sizeof(CodeT) / 16;  // 16-byte code vectors per step: 1 or 2
    for (int64_t v = (int64_t)blockIdx.x * LS_THREADS + threadIdx.x;; v += (int64_t)gridDim.x * LS_THREADS) {
        const bool in = v < n_vec;
        if (!__any(in)) break;  // wave-uniform
        uint32_t l[V], r[V], c[V];
        unsigned ok = 0;  // bit j: pair j is inside P and names rows and a code in range
#pragma unroll
        for (int j = 0; j < V; ++j) l[j] = r[j] = c[j] = 0u;
        if (in) {
            const uint4 l0 = lv[2 * v], l1 = lv[2 * v + 1], r0 = rv[2 * v], r1 = rv[2 * v + 1];
            l[0] = l0.x, l[1] = l0.y, l[2] = l0.z, l[3] = l0.w, l[4] = l1.x, l[5] = l1.y, l[6] = l1.z, l[7] = l1.w;
            r[0] = r0.x, r[1] = r0.y, r[2] = r0.z, r[3] = r0.w, r[4] = r1.x, r[5] = r1.y, r[6] = r1.z, r[7] = r1.w;
            uint4 w[CW];
#pragma unroll
            for (int j = 0; j < CW; ++j) w[j] = cv[CW * v + j];
            const CodeT *e = reinterpret_cast<const CodeT *>(w);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                c[j] = (uint32_t)e[j];
                ok |= (l[j] < A.n0 && r[j] < A.n1 && c[j] < A.n_pat ? 1u : 0u) << j;
            }
            if (ok != (1u << V) - 1u) *A.bad = 2u;
        }
        int32_t la[V], lb[V];
        double m[V], a[V], b[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            la[j] = lb[j] = -1;
            m[j] = 0.0;
            if ((ok >> j) & 1u) {
                la[j] = A.lab0[l[j]];
                lb[j] = A.lab1[r[j]];
                m[j] = A.mpat[c[j]];
            }
            tf_begin(m[j], a[j], b[j]);
        }
        for (int t = 0; t < F.n; ++t) {
            const int64_t *__restrict__ i0 = F.ids0[t];
            const int64_t *__restrict__ i1 = F.ids1[t];
            const double *__restrict__ tab = F.tab[t];
            const int64_t tab_n = F.tab_n[t];
            int64_t ia[V], ib[V];
#pragma unroll
            for (int j = 0; j < V; ++j) {
                ia[j] = ib[j] = -1;
                if ((ok >> j) & 1u) {
                    ia[j] = i0[l[j]];
                    ib[j] = i1[r[j]];
                }
            }
            double x[V];
#pragma unroll
            for (int j = 0; j < V; ++j) x[j] = tf_adj(ia[j], ib[j], tab, tab_n);  // -1: no load; an id past the table: 0.5
#pragma unroll
            for (int j = 0; j < V; ++j) tf_fold(a[j], b[j], x[j]);
        }
#pragma unroll
        for (int j = 0; j < V; ++j)
            if ((ok >> j) & 1u) score_add(cnt, A, s_th, la[j], lb[j], tf_finish(m[j], a[j], b[j]));
    }
    // tail (P not a multiple of LS_PAIRS): workgroup 0's first wave, one pair per lane
    if (blockIdx.x == 0 && threadIdx.x < 64) {
        const int64_t p = n_vec * V + lane;
        if (p < A.P) {
            const uint32_t l = (uint32_t)A.pl[p], r = (uint32_t)A.pr[p], c = (uint32_t)codes[p];
            if (l < A.n0 && r < A.n1 && c < A.n_pat)
                score_add(cnt, A, s_th, A.lab0[l], A.lab1[r], tf_pair(F, A.mpat[c], (int32_t)l, (int32_t)r, nullptr));
            else
                *A.bad = 2u;
        }
    }
    score_lds_flush(A, cnt);
}

// The survivors of a selection against the labels: one survivor per lane and step, its rows and code read coalesced
// from the selection, its score mpat[code] (SPK_SEL_MP) or per_pair[q] (SPK_SEL_TF_MP).
__global__ __launch_bounds__(LS_THREADS) void k_label_scores_sel(ScoreArgs A) {
    extern __shared__ __attribute__((aligned(16))) double s_th[];
    uint32_t *cnt = score_lds_init(A, s_th);
    for (int64_t q = (int64_t)blockIdx.x * LS_THREADS + threadIdx.x; q < A.P; q += (int64_t)gridDim.x * LS_THREADS) {
        const uint32_t l = (uint32_t)A.pl[q], r = (uint32_t)A.pr[q], c = A.code[q];
        if (l < A.n0 && r < A.n1 && c < A.n_pat)
            score_add(cnt, A, s_th, A.lab0[l], A.lab1[r], A.per_pair ? A.per_pair[q] : A.mpat[c]);
        else
            *A.bad = 2u;
    }
    score_lds_flush(A, cnt);
}

// Workgroups of either launch: wg_per_cu per CU (what the kernel's registers keep resident), never more than the
// steps there are (one at least), and never so few that one workgroup would count more than LS_BLOCK_PAIRS_MAX pairs.
static unsigned score_grid(const spk_ctx *ctx, int64_t P, int per_lane, int wg_per_cu) {
    const int64_t steps = (P / per_lane + LS_THREADS - 1) / LS_THREADS;
    int64_t g = std::min<int64_t>(steps, wg_per_cu * (int64_t)ctx->n_cu);
    g = std::max<int64_t>(g, (P + LS_BLOCK_PAIRS_MAX - 1) / LS_BLOCK_PAIRS_MAX);
    return (unsigned)std::max<int64_t>(g, 1);
}

static size_t score_lds_bytes(int T) { return (size_t)T * 8 + (size_t)3 * (T + 2) * 4; }

// The thresholds of a per-pair scoring call: 0..SPK_LABEL_SCORE_MAX_THRESHOLDS ascending doubles, no NaN.
static int check_thresholds(const char *what, int n_thresholds, const double *thresholds) {
    const std::string w(what);
    SPK_REQUIRE(n_thresholds >= 0 && n_thresholds <= SPK_LABEL_SCORE_MAX_THRESHOLDS, SPK_E_INVALID,
                w + ": 0..SPK_LABEL_SCORE_MAX_THRESHOLDS (1024) thresholds");
    SPK_REQUIRE(n_thresholds == 0 || thresholds, SPK_E_INVALID, w + ": null thresholds");
    for (int k = 0; k < n_thresholds; ++k) {
        SPK_REQUIRE(thresholds[k] == thresholds[k], SPK_E_INVALID, w + ": a threshold is NaN");
        SPK_REQUIRE(k == 0 || thresholds[k] >= thresholds[k - 1], SPK_E_INVALID, w + ": the thresholds descend");
    }
    return SPK_OK;
}

// What the spk_label_scores_* entry points share.  check(): the arguments (SPK_E_INVALID).  stage(): the label ids and
// thresholds on the device and zeroed counters.  finish(): the read-back, behind the interval's end.
struct ScoreCall {
    spk_ctx *ctx;
    const char *what;
    int T = 0;
    LabelIds L;
    DevBuf<double> thr;
    DevBuf<unsigned long long> cnt;
    StageTimer timer;
    ScoreCall(spk_ctx *c, const char *w) : ctx(c), what(w), timer{c} {}

    int check(const int64_t *ids0, const int64_t *ids1, int n_thresholds, const double *thresholds,
              const uint64_t *out_counts) {
        const std::string w(what);
        SPK_REQUIRE(ids0, SPK_E_INVALID, w + ": null label_ids0");
        SPK_REQUIRE(ctx->link_type != SPK_LINK_ONLY || ids1, SPK_E_INVALID,
                    w + ": link_only needs the right table's label_ids1");
        SPK_REQUIRE(out_counts, SPK_E_INVALID, w + ": null out_counts");
        SPK_TRY(check_thresholds(what, n_thresholds, thresholds));
        T = n_thresholds;
        return SPK_OK;
    }

    int stage(const int64_t *ids0, const int64_t *ids1, const double *thresholds, int64_t n0, int64_t n1) {
        SPK_REQUIRE((int64_t)score_lds_bytes(T) <= ctx->lds_per_block, SPK_E_LIMIT, std::string(what) + ": LDS");
        SPK_TRY(thr.alloc((size_t)T + 1));
        SPK_TRY(cnt.alloc((size_t)3 * (T + 2)));
        SPK_TRY(stage_label_ids(ctx, what, ids0, ids1, n0, n1, timer, L));
        if (T) SPK_HIP(hipMemcpyAsync(thr.p, thresholds, (size_t)T * 8, hipMemcpyHostToDevice, ctx->stream));
        return SPK_OK;
    }

    void fill(ScoreArgs &A, int64_t P, const int32_t *pl, const int32_t *pr, int64_t n0, int64_t n1) {
        A.P = P;
        A.pl = pl;
        A.pr = pr;
        A.lab0 = L.side0();
        A.lab1 = L.side1();
        A.n0 = (uint32_t)n0;
        A.n1 = (uint32_t)n1;
        A.n_pat = (uint32_t)ctx->n_patterns;
        A.T = T;
        A.top = 0;
        for (int s = 1; s <= T; s *= 2) A.top = s;
        A.thr = thr.p;
        A.gcnt = cnt.p;
        A.bad = L.bad.p;
    }

    int finish(int64_t P, uint64_t *out_counts) {
        hipStream_t st = ctx->stream;
        unsigned int h_bad = 0u;
        SPK_TRY(timer.stop());  // the read-backs are no launches
        SPK_HIP(hipMemcpyAsync(&h_bad, L.bad.p, sizeof(h_bad), hipMemcpyDeviceToHost, st));
        SPK_HIP(hipMemcpyAsync(out_counts, cnt.p, (size_t)3 * (T + 2) * 8, hipMemcpyDeviceToHost, st));
        SPK_HIP(hipStreamSynchronize(st));
        SPK_TRY(timer.add());
        SPK_REQUIRE(h_bad == 0u, SPK_E_STATE,
                    std::string(what) + ": a pair names a row outside its table or a code outside the pattern space");
        ctx->score_pairs = P;
        ctx->score_ms = timer.result();
        return SPK_OK;
    }
};

// spk_label_scores_tf*: the arguments and the state, before anything is staged.
static int scores_tf_begin(ScoreCall &C, const int64_t *label_ids0, const int64_t *label_ids1, const double *m,
                           const double *u, int n_tf_cols, bool ids_given, const double *const *adj_tables,
                           const int64_t *table_sizes, int n_thresholds, const double *thresholds,
                           const uint64_t *out_counts) {
    spk_ctx *ctx = C.ctx;
    const std::string w(C.what);
    SPK_TRY(C.check(label_ids0, label_ids1, n_thresholds, thresholds, out_counts));
    SPK_REQUIRE(m && u, SPK_E_INVALID, w + ": m and u are required");
    SPK_REQUIRE(n_tf_cols >= 1 && n_tf_cols <= 8, SPK_E_INVALID, w + ": 1..8 columns");
    SPK_REQUIRE(ids_given && adj_tables && table_sizes, SPK_E_INVALID, w + ": null arg");
    SPK_REQUIRE(ctx->codes_valid, SPK_E_STATE, w + ": no gammas");
    SPK_TRY(settle_gammas(ctx, nullptr));
    SPK_REQUIRE(ctx->codes_valid, SPK_E_STATE, w + ": no gammas");
    const int64_t P = ctx->n_pairs;
    SPK_REQUIRE(ctx->pairs_valid && ctx->pl.p && ctx->pr.p && ctx->pl.n >= (size_t)P && ctx->pr.n >= (size_t)P,
                SPK_E_STATE, w + ": no pair rows (a loaded gamma table)");
    SPK_REQUIRE(ctx->n_patterns >= 1 && ctx->n_patterns <= (int64_t)UINT32_MAX, SPK_E_LIMIT, w + ": pattern space");
    SPK_REQUIRE(ctx->table[0].n >= 0 && ctx->side_table(1).n >= 0, SPK_E_STATE, w + ": no tables");
    return SPK_OK;
}

// The counting itself, once the value ids are staged in G.
static int scores_tf_run(ScoreCall &C, TfStage &G, const int64_t *label_ids0, const int64_t *label_ids1, double lambda,
                         double one_minus, const double *m, const double *u, const double *const *adj_tables,
                         const int64_t *table_sizes, const double *thresholds, uint64_t *out_counts) {
    spk_ctx *ctx = C.ctx;
    const int64_t P = ctx->n_pairs, n0 = ctx->table[0].n, n1 = ctx->side_table(1).n;
    hipStream_t st = ctx->stream;
    SPK_TRY(tf_stage_tables(ctx, adj_tables, table_sizes, G));
    DevBuf<double> mpat;  // mp per pattern under the call's parameters: never ctx->mp
    SPK_TRY(mpat.alloc((size_t)ctx->n_patterns + 1));
    SPK_TRY(C.stage(label_ids0, label_ids1, thresholds, n0, n1));
    SPK_TRY(C.timer.open());
    SPK_TRY(pattern_mp_table(ctx, lambda, one_minus, m, u, mpat.p));
    SPK_HIP(hipMemsetAsync(C.cnt.p, 0, (size_t)3 * (C.T + 2) * 8, st));
    if (P > 0) {
        ScoreArgs A{};
        C.fill(A, P, ctx->pl.p, ctx->pr.p, n0, n1);
        A.mpat = mpat.p;
        const unsigned g = score_grid(ctx, P, LS_PAIRS, LS_WG_PER_CU);
        const size_t lds = score_lds_bytes(C.T);
        if (ctx->code_bytes == 2)
            k_label_scores_tf<uint16_t><<<g, LS_THREADS, lds, st>>>(A, G.T, reinterpret_cast<const uint16_t *>(ctx->codes.p));
        else
            k_label_scores_tf<uint32_t><<<g, LS_THREADS, lds, st>>>(A, G.T, reinterpret_cast<const uint32_t *>(ctx->codes.p));
        SPK_HIP(hipGetLastError());
    }
    return C.finish(P, out_counts);
}

// ---- pairs against a table of labelled pairs -----------------------------------------------------------------
// spk_label_pairs_histogram: k_label_hist's counting with the truth state of a pair looked up in a set of labelled
// pairs (a clerical-review sample) instead of gathered from two per-record ids.  The set is a hash table built on the
// device for the call -- open addressing, linear probing, one 64-bit word per slot; key layout, hash and capacity
// rule: include/splink_hip.h -- and probed once per candidate pair.  At 8 bytes per slot and a load of at most 0.5 the
// table of 10^5 labels is 2 MiB (L2 resident), that of 10^7 labels 256 MiB (past the Infinity Cache: every probe of
// it is an HBM gather).  An unlabelled pair, the common case, ends at the first empty slot: 2.5 slots expected at
// load 0.5, mostly in its home slot's 64-byte line.  cfg2 (46 M pairs, LDS variant), device ms of the call at 10^3 /
// 10^5 / 10^7 labels: 0.62 / 0.53 / 3.27, next to 0.19 for spk_label_histogram (profiles/ab_label_pairs.log).
constexpr unsigned long long LP_EMPTY = ~0ull;
constexpr unsigned long long LP_MATCH_BIT = 1ull << 62;
constexpr int LP_BUILD_THREADS = 256;
// Workgroups per CU of the histogram's grid, and the waves per SIMD its registers are held to (80 VGPRs: the keys,
// home slots and words of 8 pairs are live together): 3 workgroups of 8 waves are resident per CU, so every workgroup
// runs from the first cycle and takes an equal share of the steps (LS_WG_PER_CU's reasoning).
constexpr int LP_WG_PER_CU = 3;
constexpr int LP_WAVES_PER_SIMD = 6;
constexpr int64_t LP_MAX_LABELS = (int64_t)1 << 27;
// bits of the call's `bad` word.  The build's are SPK_E_INVALID, read before any pair is counted; the histogram's are
// SPK_E_STATE (the pair is not counted).
constexpr unsigned LP_BAD_ROW = 1u;     // a label names a row outside its table
constexpr unsigned LP_BAD_SELF = 2u;    // a label pairs a record with itself (one-table jobs)
constexpr unsigned LP_BAD_TWICE = 4u;   // a labelled pair given twice
constexpr unsigned LP_BAD_FLAG = 8u;    // is_match other than 0 / 1
constexpr unsigned LP_BAD_FULL = 16u;   // build: no free slot (cannot happen at load <= 0.5)
constexpr unsigned LP_BAD_PAIR = 32u;   // histogram: a pair names a row or a code out of range
constexpr unsigned LP_BAD_TABLE = 64u;  // histogram: a walk read every slot, or a slot names no label: a damaged table

struct PairTable {
    unsigned long long *slot;  // [mask + 1]: LP_EMPTY, or key | LP_MATCH_BIT if the pair is a match
    uint32_t *index;           // [mask + 1]: the label a full slot came from; read only on a hit
    uint32_t mask;             // capacity - 1
    uint32_t n_labels;
    bool ordered;              // link_only: (left row, right row) as given; otherwise (min, max)
};

// MurmurHash3's 64-bit finaliser
__device__ __forceinline__ uint64_t lp_fmix64(uint64_t k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return k;
}

// the canonical key of a pair of rows, both below 2^31
__device__ __forceinline__ uint64_t lp_key(const PairTable &T, uint32_t l, uint32_t r) {
    const uint32_t lo = T.ordered ? l : min(l, r), hi = T.ordered ? r : max(l, r);
    return (uint64_t)lo << 31 | hi;
}

// One label per thread into a table of LP_EMPTY slots.  flags[0]: the bad bits, flags[1]: the longest probe (slots an
// insert looked at, its home slot included).
__global__ __launch_bounds__(LP_BUILD_THREADS) void k_label_pairs_build(int64_t n, const int32_t *__restrict__ rows_l,
                                                                        const int32_t *__restrict__ rows_r,
                                                                        const uint8_t *__restrict__ is_match,
                                                                        uint32_t n0, uint32_t n1, PairTable T,
                                                                        unsigned int *__restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * LP_BUILD_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint32_t l = (uint32_t)rows_l[i], r = (uint32_t)rows_r[i], match = is_match[i];
    unsigned bad = 0u;
    if (l >= n0 || r >= n1) bad |= LP_BAD_ROW;
    else if (!T.ordered && l == r) bad |= LP_BAD_SELF;
    if (match > 1u) bad |= LP_BAD_FLAG;
    if (bad) {
        atomicOr(&flags[0], bad);
        return;
    }
    const uint64_t key = lp_key(T, l, r);
    const unsigned long long word = key | (match ? LP_MATCH_BIT : 0ull);
    uint32_t h = (uint32_t)lp_fmix64(key) & T.mask;
    for (uint32_t probe = 1;; ++probe) {
        const unsigned long long old = atomicCAS(&T.slot[h], LP_EMPTY, word);
        if (old == LP_EMPTY) {
            T.index[h] = (uint32_t)i;
            atomicMax(&flags[1], probe);
            return;
        }
        if ((old & ~LP_MATCH_BIT) == key) {
            atomicOr(&flags[0], LP_BAD_TWICE);
            return;
        }
        if (probe > T.mask) {  // every slot seen
            atomicOr(&flags[0], LP_BAD_FULL);
            return;
        }
        h = (h + 1u) & T.mask;
    }
}

struct PairLabelArgs {
    int64_t P;
    const int32_t *pl, *pr;
    PairTable T;
    uint32_t n0, n1;            // row counts of the pairs' left / right table
    uint32_t n_pat;
    int32_t *label_code;        // [n_labels], -1 before the launch: the largest code of a pair that hit the label; or null
    unsigned long long *ghist;  // [3 x n_pat], zeroed before the launch
    unsigned int *bad;
};

// The walk of one pair from its home slot h, whose word w is loaded already: the pair's bin, or in = false when the
// table is damaged.  At most capacity slots are read, so no wave can spin.
__device__ __forceinline__ uint32_t lp_bin(const PairLabelArgs &A, uint64_t key, uint32_t h, unsigned long long w,
                                           uint32_t c, bool &in) {
    if (!in) return 0xFFFFFFFFu;
    uint32_t state = (uint32_t)SPK_LABEL_UNKNOWN;
    for (uint32_t left = A.T.mask; w != LP_EMPTY; --left) {  // left: slots the walk may still move on to
        if ((w & ~LP_MATCH_BIT) == key) {
            const uint32_t at = A.T.index[h];
            if (at >= A.T.n_labels) break;  // a slot that names no label
            state = (uint32_t)((w >> 62) & 1ull);
            if (A.label_code) atomicMax(&A.label_code[at], (int32_t)c);
            return state * A.n_pat + c;
        }
        if (left == 0u) break;  // every slot read
        h = (h + 1u) & A.T.mask;
        w = A.T.slot[h];
    }
    if (w == LP_EMPTY) return state * A.n_pat + c;  // no label: the loop ended, it was not left by a break
    atomicOr(A.bad, LP_BAD_TABLE);
    in = false;
    return 0xFFFFFFFFu;
}

// The same walk for the kernels that score the pair themselves (spk_label_pairs_scores_*): the pair's truth state and
// in `at` the label it hit (LP_NO_LABEL: none), or LP_DAMAGED for a table that is damaged.  The same bound.
constexpr uint32_t LP_NO_LABEL = 0xFFFFFFFFu;
constexpr uint32_t LP_DAMAGED = (uint32_t)SPK_LABEL_STATES;
__device__ __forceinline__ uint32_t lp_walk(const PairTable &T, uint64_t key, uint32_t h, unsigned long long w,
                                            uint32_t &at) {
    at = LP_NO_LABEL;
    for (uint32_t left = T.mask; w != LP_EMPTY; --left) {  // left: slots the walk may still move on to
        if ((w & ~LP_MATCH_BIT) == key) {
            const uint32_t i = T.index[h];
            if (i >= T.n_labels) return LP_DAMAGED;  // a slot that names no label
            at = i;
            return (uint32_t)((w >> 62) & 1ull);
        }
        if (left == 0u) return LP_DAMAGED;  // every slot read
        h = (h + 1u) & T.mask;
        w = T.slot[h];
    }
    return (uint32_t)SPK_LABEL_UNKNOWN;
}

// k_label_hist with the two label gathers replaced by the probe: the same 8 pairs per lane and step, the same tail
// wave, label_add and LDS flush.  Per step a lane first issues the home-slot loads of all its pairs, so that they are in
// flight together as k_label_hist's gathers are, and only then walks on where a home slot held another key.
template <typename CodeT, bool LDS>
__global__ __launch_bounds__(LH_THREADS, LP_WAVES_PER_SIMD) void k_label_pairs_hist(PairLabelArgs A,
                                                                                   const CodeT *__restrict__ codes) {
    extern __shared__ uint32_t sh[];
    const int n_bins = 3 * (int)A.n_pat;
    if (LDS) {
        for (int b = threadIdx.x; b < n_bins; b += LH_THREADS) sh[b] = 0;
        __syncthreads();
    }
    const int lane = threadIdx.x & 63;
    const int64_t n_vec = A.P / LH_PAIRS;
    const uint4 *lv = reinterpret_cast<const uint4 *>(A.pl);
    const uint4 *rv = reinterpret_cast<const uint4 *>(A.pr);
    const uint4 *cv = reinterpret_cast<const uint4 *>(codes);
    constexpr int CW = LH_PAIRS * (int)sizeof(CodeT) / 16;  // 16-byte code vectors per step: 1 or 2
    for (int64_t v = (int64_t)blockIdx.x * LH_THREADS + threadIdx.x;; v += (int64_t)gridDim.x * LH_THREADS) {
        const bool in = v < n_vec;
        if (!__any(in)) break;  // wave-uniform: every lane stays inside the ballots of label_add
        uint32_t l[LH_PAIRS], r[LH_PAIRS], c[LH_PAIRS], h[LH_PAIRS], bin[LH_PAIRS];
        uint64_t key[LH_PAIRS];
        unsigned long long w[LH_PAIRS];
        bool ok[LH_PAIRS];
#pragma unroll
        for (int j = 0; j < LH_PAIRS; ++j) l[j] = r[j] = c[j] = 0xFFFFFFFFu;
        if (in) {
            const uint4 l0 = lv[2 * v], l1 = lv[2 * v + 1], r0 = rv[2 * v], r1 = rv[2 * v + 1];
            l[0] = l0.x, l[1] = l0.y, l[2] = l0.z, l[3] = l0.w, l[4] = l1.x, l[5] = l1.y, l[6] = l1.z, l[7] = l1.w;
            r[0] = r0.x, r[1] = r0.y, r[2] = r0.z, r[3] = r0.w, r[4] = r1.x, r[5] = r1.y, r[6] = r1.z, r[7] = r1.w;
            uint4 x[CW];
#pragma unroll
            for (int j = 0; j < CW; ++j) x[j] = cv[CW * v + j];
            const CodeT *e = reinterpret_cast<const CodeT *>(x);
#pragma unroll
            for (int j = 0; j < LH_PAIRS; ++j) c[j] = (uint32_t)e[j];
        }
#pragma unroll
        for (int j = 0; j < LH_PAIRS; ++j) {  // all the home slots first
            ok[j] = in && l[j] < A.n0 && r[j] < A.n1 && c[j] < A.n_pat;
            if (in && !ok[j]) atomicOr(A.bad, LP_BAD_PAIR);
            key[j] = lp_key(A.T, l[j], r[j]);
            h[j] = (uint32_t)lp_fmix64(key[j]) & A.T.mask;
            w[j] = ok[j] ? A.T.slot[h[j]] : LP_EMPTY;
        }
#pragma unroll
        for (int j = 0; j < LH_PAIRS; ++j) bin[j] = lp_bin(A, key[j], h[j], w[j], c[j], ok[j]);
#pragma unroll
        for (int j = 0; j < LH_PAIRS; ++j) label_add<LDS>(bin[j], ok[j], lane, sh, A.ghist);
    }
    // tail (P not a multiple of LH_PAIRS): workgroup 0's first wave, one pair per lane, every lane in the ballots
    if (blockIdx.x == 0 && threadIdx.x < 64) {
        const int64_t p = n_vec * LH_PAIRS + lane;
        const bool in = p < A.P;
        const uint32_t l = in ? (uint32_t)A.pl[p] : 0u, r = in ? (uint32_t)A.pr[p] : 0u, c = in ? (uint32_t)codes[p] : 0u;
        bool ok = in && l < A.n0 && r < A.n1 && c < A.n_pat;
        if (in && !ok) atomicOr(A.bad, LP_BAD_PAIR);
        const uint64_t key = lp_key(A.T, l, r);
        const uint32_t h = (uint32_t)lp_fmix64(key) & A.T.mask;
        const uint32_t bin = lp_bin(A, key, h, ok ? A.T.slot[h] : LP_EMPTY, c, ok);
        label_add<LDS>(bin, ok, lane, sh, A.ghist);
    }
    if (LDS) {
        __syncthreads();
        for (int b = threadIdx.x; b < n_bins; b += LH_THREADS) {
            const uint32_t n = sh[b];
            if (n) atomicAdd(&A.ghist[b], (unsigned long long)n);
        }
    }
}

template <typename CodeT>
static int launch_label_pairs_hist(spk_ctx *ctx, const PairLabelArgs &A, bool lds) {
    const unsigned g = label_grid(ctx, A.P, LP_WG_PER_CU);
    const CodeT *codes = reinterpret_cast<const CodeT *>(ctx->codes.p);
    if (lds) k_label_pairs_hist<CodeT, true><<<g, LH_THREADS, (size_t)3 * A.n_pat * 4, ctx->stream>>>(A, codes);
    else k_label_pairs_hist<CodeT, false><<<g, LH_THREADS, 0, ctx->stream>>>(A, codes);
    SPK_HIP(hipGetLastError());
    return SPK_OK;
}

// The table of labelled pairs of one call on the device: locals of the entry points that look pairs up in it.
struct PairTableStage {
    DevBuf<unsigned long long> slot;
    DevBuf<uint32_t> index;
    DevBuf<int32_t> d_l, d_r;
    DevBuf<uint8_t> d_match;
    DevBuf<unsigned int> flags;  // [0] the bad bits (0 after a good build: the counting kernels' from then on), [1] the
                                 // longest insert probe
    int64_t capacity = 0;
    int max_probe = 0;
    PairTable tab{};
};

// Uploads the labels, clears the table and inserts them (k_label_pairs_build, inside T's intervals; the uploads are no
// launches: outside them), then reads the flags back: what is wrong with the labels is SPK_E_INVALID under `what`,
// known before a pair is counted.  Leaves S.flags[0] = 0 and the stream synchronised.
static int stage_pair_table(spk_ctx *ctx, const char *what, int64_t n_labels, const int32_t *rows_l,
                            const int32_t *rows_r, const uint8_t *is_match, int64_t n0, int64_t n1, StageTimer &T,
                            PairTableStage &S) {
    const std::string w(what);
    hipStream_t st = ctx->stream;
    S.capacity = 64;
    while (S.capacity < 2 * n_labels) S.capacity *= 2;
    SPK_TRY(S.slot.alloc((size_t)S.capacity));
    SPK_TRY(S.index.alloc((size_t)S.capacity));
    SPK_TRY(S.flags.alloc(2));
    S.tab = PairTable{S.slot.p, S.index.p, (uint32_t)(S.capacity - 1), (uint32_t)n_labels,
                      ctx->link_type == SPK_LINK_ONLY};
    if (n_labels > 0) {
        SPK_TRY(S.d_l.alloc((size_t)n_labels));
        SPK_TRY(S.d_r.alloc((size_t)n_labels));
        SPK_TRY(S.d_match.alloc((size_t)n_labels));
        SPK_HIP(hipMemcpyAsync(S.d_l.p, rows_l, (size_t)n_labels * 4, hipMemcpyHostToDevice, st));
        SPK_HIP(hipMemcpyAsync(S.d_r.p, rows_r, (size_t)n_labels * 4, hipMemcpyHostToDevice, st));
        SPK_HIP(hipMemcpyAsync(S.d_match.p, is_match, (size_t)n_labels, hipMemcpyHostToDevice, st));
    }
    SPK_TRY(T.open());
    SPK_HIP(hipMemsetAsync(S.flags.p, 0, 2 * sizeof(unsigned int), st));
    SPK_HIP(hipMemsetAsync(S.slot.p, 0xFF, (size_t)S.capacity * 8, st));
    if (n_labels > 0) {
        k_label_pairs_build<<<(unsigned)((n_labels + LP_BUILD_THREADS - 1) / LP_BUILD_THREADS), LP_BUILD_THREADS, 0,
                              st>>>(n_labels, S.d_l.p, S.d_r.p, S.d_match.p, (uint32_t)n0, (uint32_t)n1, S.tab,
                                    S.flags.p);
        SPK_HIP(hipGetLastError());
    }
    SPK_TRY(T.stop());
    unsigned int h_flags[2] = {0u, 0u};
    SPK_HIP(hipMemcpyAsync(h_flags, S.flags.p, sizeof(h_flags), hipMemcpyDeviceToHost, st));
    SPK_HIP(hipStreamSynchronize(st));
    SPK_TRY(T.add());
    SPK_REQUIRE(!(h_flags[0] & LP_BAD_FLAG), SPK_E_INVALID, w + ": an is_match other than 0 or 1");
    SPK_REQUIRE(!(h_flags[0] & LP_BAD_ROW), SPK_E_INVALID, w + ": a labelled pair names a row outside its table");
    SPK_REQUIRE(!(h_flags[0] & LP_BAD_SELF), SPK_E_INVALID, w + ": a labelled pair of a record with itself");
    SPK_REQUIRE(!(h_flags[0] & LP_BAD_TWICE), SPK_E_INVALID, w + ": a labelled pair given twice");
    SPK_REQUIRE(h_flags[0] == 0u, SPK_E_STATE, w + ": the pair table is full");
    S.max_probe = (int)h_flags[1];
    return SPK_OK;
}

// ---- scores against a table of labelled pairs, per pair ------------------------------------------------------
// spk_label_pairs_scores_*: the counting of spk_label_scores_* with the truth state of a pair looked up in the table
// of spk_label_pairs_histogram instead of gathered from two per-record ids.  The same thresholds, bins, LDS counters
// and flush (score_lds_init / score_bin / score_lds_flush); the same table, key, hash and bounded walk (lp_key /
// lp_fmix64 / lp_walk).  A pair that hits label i also raises found[i] to 1 + its index (a 64-bit atomicMax), and
// a second launch, one thread per label, scores exactly the pair found: a hand-loaded pair set that repeats a
// labelled pair gives the largest index whatever the arrival order, and no score is written from a race.
//
// Pairs per lane and step (4 or 8), and the waves per SIMD the registers are held to, which is also the workgroups
// per CU the grid is capped at (compile-time switches for tools/ab_label_pair_scores.py's A/B).  The keys, home slots
// and words of the probe are dead before the tf fold starts, so the union costs no more registers than the fold: 128
// VGPRs with 8 pairs per lane (4 waves per SIMD), 70 with 4 (7 waves), no scratch in either; held to 8 waves (64
// VGPRs) the 4-pair form spills 20 bytes and is not offered.  The pass is bound by the latency of its dependent
// gathers (probe, then value ids, then table entries), so resident waves win over pairs per lane.  cfg2 (46 M
// pairs), device ms of the call at T = 72 with 10^3 / 10^5 / 10^7 labels: 8 pairs at 3 waves 1.09 / 0.95 / 4.11, at 4
// waves 0.93 / 0.83 / 3.94; 4 pairs at 4 waves 1.03 / 0.91 / 3.89, at 6 waves 0.86 / 0.76 / 3.71
// (profiles/ab_label_pair_scores.log).
#ifndef SPK_LABEL_PAIR_SCORE_PAIRS
#define SPK_LABEL_PAIR_SCORE_PAIRS 4
#endif
#ifndef SPK_LABEL_PAIR_SCORE_WAVES
#define SPK_LABEL_PAIR_SCORE_WAVES 6
#endif
constexpr int LPS_PAIRS = SPK_LABEL_PAIR_SCORE_PAIRS;
constexpr int LPS_WAVES_PER_SIMD = SPK_LABEL_PAIR_SCORE_WAVES;  // = workgroups per CU: a workgroup puts one wave on each SIMD
constexpr int LPS_SEL_WG_PER_CU = 8;
static_assert(LPS_PAIRS == 4 || LPS_PAIRS == 8, "4 or 8 pairs per lane");

struct PairScoreArgs {
    ScoreArgs S;                // lab0 / lab1 are not read; *S.bad takes the LP_BAD_* bits
    PairTable T;
    unsigned long long *found;  // [n_labels], zeroed before the launch: 1 + the largest index of a pair that hit the
                                // label; or null
};

__device__ __forceinline__ void score_add_state(uint32_t *cnt, const ScoreArgs &A, const double *th, uint32_t state,
                                                double s) {
    atomicAdd(&cnt[state * ((uint32_t)A.T + 2u) + score_bin(s, th, (uint32_t)A.T, A.top)], 1u);
}

// V consecutive codes of step v, coalesced: 8, 16 or 32 bytes per lane
template <typename CodeT, int V>
__device__ __forceinline__ void lps_load_codes(const CodeT *__restrict__ codes, int64_t v, uint32_t (&c)[V]) {
    constexpr int BYTES = V * (int)sizeof(CodeT);
    if constexpr (BYTES == 8) {
        const uint2 w = reinterpret_cast<const uint2 *>(codes)[v];
        c[0] = w.x & 0xFFFFu, c[1] = w.x >> 16, c[2] = w.y & 0xFFFFu, c[3] = w.y >> 16;
    } else {
        constexpr int CW = BYTES / 16;
        uint4 w[CW];
#pragma unroll
        for (int j = 0; j < CW; ++j) w[j] = reinterpret_cast<const uint4 *>(codes)[CW * v + j];
        const CodeT *e = reinterpret_cast<const CodeT *>(w);
#pragma unroll
        for (int j = 0; j < V; ++j) c[j] = (uint32_t)e[j];
    }
}

// Every pair of the context against the table, by tf_adjusted_match_prob: k_label_scores_tf's loop with the two label
// gathers replaced by k_label_pairs_hist's probe.  Per step a lane issues the home-slot loads and the mp gathers of
// all its pairs together, walks on only where a home slot held another key (lp_walk: bounded by the capacity), and
// then folds the tf columns as k_label_scores_tf does.  The states of the lane's pairs are packed two bits each.
template <typename CodeT, int V>
__global__ __launch_bounds__(LS_THREADS, LPS_WAVES_PER_SIMD) void k_label_pairs_scores_tf(
    PairScoreArgs B, TfApply F, const CodeT *__restrict__ codes) {
    extern __shared__ __attribute__((aligned(16))) double s_th[];
    const ScoreArgs &A = B.S;
    uint32_t *cnt = score_lds_init(A, s_th);
    const int lane = threadIdx.x & 63;
    const int64_t n_vec = A.P / V;
    const uint4 *lv = reinterpret_cast<const uint4 *>(A.pl);
    const uint4 *rv = reinterpret_cast<const uint4 *>(A.pr);
    constexpr int RW = V / 4;  // 16-byte row vectors per side and step
    for (int64_t v = (int64_t)blockIdx.x * LS_THREADS + threadIdx.x;; v += (int64_t)gridDim.x * LS_THREADS) {
        const bool in = v < n_vec;
        if (!__any(in)) break;  // wave-uniform
        uint32_t l[V], r[V], c[V];
        unsigned ok = 0;  // bit j: pair j is inside P and names rows and a code in range
#pragma unroll
        for (int j = 0; j < V; ++j) l[j] = r[j] = c[j] = 0u;
        if (in) {
#pragma unroll
            for (int k = 0; k < RW; ++k) {
                const uint4 a = lv[RW * v + k], b = rv[RW * v + k];
                l[4 * k] = a.x, l[4 * k + 1] = a.y, l[4 * k + 2] = a.z, l[4 * k + 3] = a.w;
                r[4 * k] = b.x, r[4 * k + 1] = b.y, r[4 * k + 2] = b.z, r[4 * k + 3] = b.w;
            }
            lps_load_codes<CodeT, V>(codes, v, c);
#pragma unroll
            for (int j = 0; j < V; ++j) ok |= (l[j] < A.n0 && r[j] < A.n1 && c[j] < A.n_pat ? 1u : 0u) << j;
            if (ok != (1u << V) - 1u) atomicOr(A.bad, LP_BAD_PAIR);
        }
        double m[V], a[V], b[V];
        unsigned states = 0;  // two bits per pair
        {
            uint64_t key[V];
            uint32_t h[V];
            unsigned long long w[V];
#pragma unroll
            for (int j = 0; j < V; ++j) {  // all the home slots and the mp gathers first
                key[j] = lp_key(B.T, l[j], r[j]);
                h[j] = (uint32_t)lp_fmix64(key[j]) & B.T.mask;
                w[j] = LP_EMPTY;
                m[j] = 0.0;
                if ((ok >> j) & 1u) {
                    w[j] = B.T.slot[h[j]];
                    m[j] = A.mpat[c[j]];
                }
            }
#pragma unroll
            for (int j = 0; j < V; ++j) {
                uint32_t at;
                const uint32_t s = lp_walk(B.T, key[j], h[j], w[j], at);
                if (s == LP_DAMAGED) {  // the pair is not counted
                    atomicOr(A.bad, LP_BAD_TABLE);
                    ok &= ~(1u << j);
                } else if (at != LP_NO_LABEL && B.found) {
                    atomicMax(&B.found[at], (unsigned long long)(v * V + j) + 1ull);
                }
                states |= (s & 3u) << (2 * j);
            }
        }
#pragma unroll
        for (int j = 0; j < V; ++j) tf_begin(m[j], a[j], b[j]);
        for (int t = 0; t < F.n; ++t) {
            const int64_t *__restrict__ i0 = F.ids0[t];
            const int64_t *__restrict__ i1 = F.ids1[t];
            const double *__restrict__ tab = F.tab[t];
            const int64_t tab_n = F.tab_n[t];
            int64_t ia[V], ib[V];
#pragma unroll
            for (int j = 0; j < V; ++j) {
                ia[j] = ib[j] = -1;
                if ((ok >> j) & 1u) {
                    ia[j] = i0[l[j]];
                    ib[j] = i1[r[j]];
                }
            }
            double x[V];
#pragma unroll
            for (int j = 0; j < V; ++j) x[j] = tf_adj(ia[j], ib[j], tab, tab_n);  // -1: no load; an id past the table: 0.5
#pragma unroll
            for (int j = 0; j < V; ++j) tf_fold(a[j], b[j], x[j]);
        }
#pragma unroll
        for (int j = 0; j < V; ++j)
            if ((ok >> j) & 1u) score_add_state(cnt, A, s_th, (states >> (2 * j)) & 3u, tf_finish(m[j], a[j], b[j]));
    }
    // tail (P not a multiple of V): workgroup 0's first wave, one pair per lane
    if (blockIdx.x == 0 && threadIdx.x < 64) {
        const int64_t p = n_vec * V + lane;
        if (p < A.P) {
            const uint32_t l = (uint32_t)A.pl[p], r = (uint32_t)A.pr[p], c = (uint32_t)codes[p];
            if (l < A.n0 && r < A.n1 && c < A.n_pat) {
                const uint64_t key = lp_key(B.T, l, r);
                const uint32_t h = (uint32_t)lp_fmix64(key) & B.T.mask;
                uint32_t at;
                const uint32_t s = lp_walk(B.T, key, h, B.T.slot[h], at);
                if (s == LP_DAMAGED) {
                    atomicOr(A.bad, LP_BAD_TABLE);
                } else {
                    if (at != LP_NO_LABEL && B.found) atomicMax(&B.found[at], (unsigned long long)p + 1ull);
                    score_add_state(cnt, A, s_th, s, tf_pair(F, A.mpat[c], (int32_t)l, (int32_t)r, nullptr));
                }
            } else {
                atomicOr(A.bad, LP_BAD_PAIR);
            }
        }
    }
    score_lds_flush(A, cnt);
}

// The survivors of a selection against the table: k_label_scores_sel with the same replacement.
__global__ __launch_bounds__(LS_THREADS) void k_label_pairs_scores_sel(PairScoreArgs B) {
    extern __shared__ __attribute__((aligned(16))) double s_th[];
    const ScoreArgs &A = B.S;
    uint32_t *cnt = score_lds_init(A, s_th);
    for (int64_t q = (int64_t)blockIdx.x * LS_THREADS + threadIdx.x; q < A.P; q += (int64_t)gridDim.x * LS_THREADS) {
        const uint32_t l = (uint32_t)A.pl[q], r = (uint32_t)A.pr[q], c = A.code[q];
        if (l < A.n0 && r < A.n1 && c < A.n_pat) {
            const uint64_t key = lp_key(B.T, l, r);
            const uint32_t h = (uint32_t)lp_fmix64(key) & B.T.mask;
            uint32_t at;
            const uint32_t s = lp_walk(B.T, key, h, B.T.slot[h], at);
            if (s == LP_DAMAGED) {
                atomicOr(A.bad, LP_BAD_TABLE);
            } else {
                if (at != LP_NO_LABEL && B.found) atomicMax(&B.found[at], (unsigned long long)q + 1ull);
                score_add_state(cnt, A, s_th, s, A.per_pair ? A.per_pair[q] : A.mpat[c]);
            }
        } else {
            atomicOr(A.bad, LP_BAD_PAIR);
        }
    }
    score_lds_flush(A, cnt);
}

// One label per thread, after the counting: the index of the pair found (-1: none) and the score of exactly that
// pair (NaN: none), by tf_pair over the context's pairs and codes (tf) or from the selection's own scores (codes =
// the survivors' codes).  found[i] was only raised by pairs that the counting kernel found in range.
template <typename CodeT>
__global__ __launch_bounds__(LP_BUILD_THREADS) void k_label_pairs_scores_found(int64_t n, PairScoreArgs B, bool tf,
                                                                               TfApply F,
                                                                               const CodeT *__restrict__ codes,
                                                                               int64_t *__restrict__ out_pair,
                                                                               double *__restrict__ out_score) {
    const int64_t i = (int64_t)blockIdx.x * LP_BUILD_THREADS + threadIdx.x;
    if (i >= n) return;
    const ScoreArgs &A = B.S;
    const int64_t q = (int64_t)B.found[i] - 1;
    double s = NAN;
    if (q >= 0 && q < A.P) {
        if (tf) s = tf_pair(F, A.mpat[(uint32_t)codes[q]], A.pl[q], A.pr[q], nullptr);
        else s = A.per_pair ? A.per_pair[q] : A.mpat[(uint32_t)codes[q]];
    }
    out_pair[i] = q < A.P ? q : -1;
    out_score[i] = s;
}

// What the spk_label_pairs_scores_* entry points share.  check(): the arguments (SPK_E_INVALID).  stage(): the table
// of labelled pairs (stage_pair_table: the label faults), the thresholds and the per-label words on the device.
// count_from(): zeroed counters and words inside the open interval.  finish(): the per-label launch and the read-back.
struct PairScoreCall {
    spk_ctx *ctx;
    const char *what;
    int T = 0;
    int64_t n_labels = 0;
    bool per_label = false;  // out_label_pair or out_label_score is wanted
    PairTableStage tab;
    DevBuf<double> thr, d_score;
    DevBuf<unsigned long long> cnt, found;
    DevBuf<int64_t> d_pair;
    StageTimer timer;
    PairScoreCall(spk_ctx *c, const char *w) : ctx(c), what(w), timer{c} {}

    int check(int64_t n, const int32_t *rows_l, const int32_t *rows_r, const uint8_t *is_match, int n_thresholds,
              const double *thresholds, const uint64_t *out_counts, const int64_t *out_pair, const double *out_score) {
        const std::string w(what);
        SPK_REQUIRE(n >= 0, SPK_E_INVALID, w + ": negative n_labels");
        SPK_REQUIRE(n == 0 || (rows_l && rows_r && is_match), SPK_E_INVALID, w + ": null rows_l, rows_r or is_match");
        SPK_REQUIRE(out_counts, SPK_E_INVALID, w + ": null out_counts");
        SPK_TRY(check_thresholds(what, n_thresholds, thresholds));
        T = n_thresholds;
        n_labels = n;
        per_label = n > 0 && (out_pair || out_score);
        return SPK_OK;
    }

    int stage(const int32_t *rows_l, const int32_t *rows_r, const uint8_t *is_match, const double *thresholds,
              int64_t n0, int64_t n1) {
        SPK_REQUIRE(n_labels <= LP_MAX_LABELS, SPK_E_LIMIT, std::string(what) + ": more than 2^27 labelled pairs");
        SPK_REQUIRE((int64_t)score_lds_bytes(T) <= ctx->lds_per_block, SPK_E_LIMIT, std::string(what) + ": LDS");
        SPK_TRY(thr.alloc((size_t)T + 1));
        SPK_TRY(cnt.alloc((size_t)3 * (T + 2)));
        if (per_label) {
            SPK_TRY(found.alloc((size_t)n_labels));
            SPK_TRY(d_pair.alloc((size_t)n_labels));
            SPK_TRY(d_score.alloc((size_t)n_labels));
        }
        SPK_TRY(stage_pair_table(ctx, what, n_labels, rows_l, rows_r, is_match, n0, n1, timer, tab));
        if (T) SPK_HIP(hipMemcpyAsync(thr.p, thresholds, (size_t)T * 8, hipMemcpyHostToDevice, ctx->stream));
        return SPK_OK;
    }

    int clear() {  // inside the open interval
        SPK_HIP(hipMemsetAsync(cnt.p, 0, (size_t)3 * (T + 2) * 8, ctx->stream));
        if (per_label) SPK_HIP(hipMemsetAsync(found.p, 0, (size_t)n_labels * 8, ctx->stream));
        return SPK_OK;
    }

    void fill(PairScoreArgs &B, int64_t P, const int32_t *pl, const int32_t *pr, int64_t n0, int64_t n1) {
        ScoreArgs &A = B.S;
        A.P = P;
        A.pl = pl;
        A.pr = pr;
        A.n0 = (uint32_t)n0;
        A.n1 = (uint32_t)n1;
        A.n_pat = (uint32_t)ctx->n_patterns;
        A.T = T;
        A.top = 0;
        for (int s = 1; s <= T; s *= 2) A.top = s;
        A.thr = thr.p;
        A.gcnt = cnt.p;
        A.bad = tab.flags.p;
        B.T = tab.tab;
        B.found = per_label ? found.p : nullptr;
    }

    // The per-label launch (tf: by tf_pair over `codes`, the context's; else from the selection's scores and codes).
    template <typename CodeT>
    int per_label_launch(const PairScoreArgs &B, bool tf, const TfApply &F, const CodeT *codes) {
        if (!per_label) return SPK_OK;
        k_label_pairs_scores_found<CodeT><<<(unsigned)((n_labels + LP_BUILD_THREADS - 1) / LP_BUILD_THREADS),
                                            LP_BUILD_THREADS, 0, ctx->stream>>>(n_labels, B, tf, F, codes, d_pair.p,
                                                                                 d_score.p);
        SPK_HIP(hipGetLastError());
        return SPK_OK;
    }

    int finish(int64_t P, uint64_t *out_counts, int64_t *out_pair, double *out_score) {
        hipStream_t st = ctx->stream;
        const std::string w(what);
        unsigned int h_bad = 0u;
        SPK_TRY(timer.stop());  // the read-backs are no launches
        SPK_HIP(hipMemcpyAsync(&h_bad, tab.flags.p, sizeof(h_bad), hipMemcpyDeviceToHost, st));
        SPK_HIP(hipMemcpyAsync(out_counts, cnt.p, (size_t)3 * (T + 2) * 8, hipMemcpyDeviceToHost, st));
        if (per_label && out_pair)
            SPK_HIP(hipMemcpyAsync(out_pair, d_pair.p, (size_t)n_labels * 8, hipMemcpyDeviceToHost, st));
        if (per_label && out_score)
            SPK_HIP(hipMemcpyAsync(out_score, d_score.p, (size_t)n_labels * 8, hipMemcpyDeviceToHost, st));
        SPK_HIP(hipStreamSynchronize(st));
        SPK_TRY(timer.add());
        SPK_REQUIRE(!(h_bad & LP_BAD_PAIR), SPK_E_STATE,
                    w + ": a pair names a row outside its table or a code outside the pattern space");
        SPK_REQUIRE(h_bad == 0u, SPK_E_STATE, w + ": the pair table is damaged");
        ctx->lpscore_pairs = P;
        ctx->lpscore_ms = timer.result();
        ctx->lpscore_capacity = tab.capacity;
        ctx->lpscore_max_probe = tab.max_probe;
        return SPK_OK;
    }
};

// spk_label_pairs_scores_tf*: the arguments and the state, before anything is staged (scores_tf_begin's rules).
static int pair_scores_tf_begin(PairScoreCall &C, int64_t n_labels, const int32_t *rows_l, const int32_t *rows_r,
                                const uint8_t *is_match, const double *m, const double *u, int n_tf_cols,
                                bool ids_given, const double *const *adj_tables, const int64_t *table_sizes,
                                int n_thresholds, const double *thresholds, const uint64_t *out_counts,
                                const int64_t *out_pair, const double *out_score) {
    spk_ctx *ctx = C.ctx;
    const std::string w(C.what);
    SPK_TRY(C.check(n_labels, rows_l, rows_r, is_match, n_thresholds, thresholds, out_counts, out_pair, out_score));
    SPK_REQUIRE(m && u, SPK_E_INVALID, w + ": m and u are required");
    SPK_REQUIRE(n_tf_cols >= 1 && n_tf_cols <= 8, SPK_E_INVALID, w + ": 1..8 columns");
    SPK_REQUIRE(ids_given && adj_tables && table_sizes, SPK_E_INVALID, w + ": null arg");
    SPK_REQUIRE(ctx->codes_valid, SPK_E_STATE, w + ": no gammas");
    SPK_TRY(settle_gammas(ctx, nullptr));
    SPK_REQUIRE(ctx->codes_valid, SPK_E_STATE, w + ": no gammas");
    const int64_t P = ctx->n_pairs;
    SPK_REQUIRE(ctx->pairs_valid && ctx->pl.p && ctx->pr.p && ctx->pl.n >= (size_t)P && ctx->pr.n >= (size_t)P,
                SPK_E_STATE, w + ": no pair rows (a loaded gamma table)");
    SPK_REQUIRE(ctx->n_patterns >= 1 && ctx->n_patterns <= (int64_t)UINT32_MAX, SPK_E_LIMIT, w + ": pattern space");
    SPK_REQUIRE(ctx->table[0].n >= 0 && ctx->side_table(1).n >= 0, SPK_E_STATE, w + ": no tables");
    return SPK_OK;
}

// The counting itself, once the value ids are staged in G.
static int pair_scores_tf_run(PairScoreCall &C, TfStage &G, const int32_t *rows_l, const int32_t *rows_r,
                              const uint8_t *is_match, double lambda, double one_minus, const double *m,
                              const double *u, const double *const *adj_tables, const int64_t *table_sizes,
                              const double *thresholds, uint64_t *out_counts, int64_t *out_pair, double *out_score) {
    spk_ctx *ctx = C.ctx;
    const int64_t P = ctx->n_pairs, n0 = ctx->table[0].n, n1 = ctx->side_table(1).n;
    hipStream_t st = ctx->stream;
    SPK_TRY(tf_stage_tables(ctx, adj_tables, table_sizes, G));
    DevBuf<double> mpat;  // mp per pattern under the call's parameters: never ctx->mp
    SPK_TRY(mpat.alloc((size_t)ctx->n_patterns + 1));
    SPK_TRY(C.stage(rows_l, rows_r, is_match, thresholds, n0, n1));
    SPK_TRY(C.timer.open());
    SPK_TRY(pattern_mp_table(ctx, lambda, one_minus, m, u, mpat.p));
    SPK_TRY(C.clear());
    PairScoreArgs B{};
    C.fill(B, P, ctx->pl.p, ctx->pr.p, n0, n1);
    B.S.mpat = mpat.p;
    const unsigned g = score_grid(ctx, P, LPS_PAIRS, LPS_WAVES_PER_SIMD);
    const size_t lds = score_lds_bytes(C.T);
    if (ctx->code_bytes == 2) {
        const uint16_t *codes = reinterpret_cast<const uint16_t *>(ctx->codes.p);
        if (P > 0) k_label_pairs_scores_tf<uint16_t, LPS_PAIRS><<<g, LS_THREADS, lds, st>>>(B, G.T, codes);
        SPK_HIP(hipGetLastError());
        SPK_TRY(C.per_label_launch<uint16_t>(B, true, G.T, codes));
    } else {
        const uint32_t *codes = reinterpret_cast<const uint32_t *>(ctx->codes.p);
        if (P > 0) k_label_pairs_scores_tf<uint32_t, LPS_PAIRS><<<g, LS_THREADS, lds, st>>>(B, G.T, codes);
        SPK_HIP(hipGetLastError());
        SPK_TRY(C.per_label_launch<uint32_t>(B, true, G.T, codes));
    }
    return C.finish(P, out_counts, out_pair, out_score);
}

}  // namespace spk

using namespace spk;

extern "C" int spk_label_histogram(spk_ctx *ctx, const int64_t *ids_side0, const int64_t *ids_side1, double lambda,
                                   double one_minus, const double *m, const double *u, uint64_t *out_counts,
                                   double *out_pattern_mp) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "spk_label_histogram: null ctx");
    SPK_HIP(hipSetDevice(ctx->device));
    ctx->label_pairs = -1;
    ctx->label_ms = -1.0;
    const bool two = ctx->link_type == SPK_LINK_ONLY;
    SPK_REQUIRE(ids_side0, SPK_E_INVALID, "spk_label_histogram: null ids_side0");
    SPK_REQUIRE(!two || ids_side1, SPK_E_INVALID, "spk_label_histogram: link_only needs the right table's ids_side1");
    SPK_REQUIRE(out_counts, SPK_E_INVALID, "spk_label_histogram: null out_counts");
    SPK_REQUIRE((m == nullptr) == (u == nullptr), SPK_E_INVALID, "spk_label_histogram: m and u come together");
    SPK_REQUIRE(!out_pattern_mp || (m && u), SPK_E_INVALID, "spk_label_histogram: out_pattern_mp needs m and u");
    SPK_REQUIRE(ctx->codes_valid, SPK_E_STATE, "spk_label_histogram: no gammas");
    SPK_TRY(settle_gammas(ctx, nullptr));
    SPK_REQUIRE(ctx->codes_valid, SPK_E_STATE, "spk_label_histogram: no gammas");
    const int64_t P = ctx->n_pairs, n_pat = ctx->n_patterns;
    SPK_REQUIRE(ctx->pairs_valid && ctx->pl.p && ctx->pr.p && ctx->pl.n >= (size_t)P && ctx->pr.n >= (size_t)P,
                SPK_E_STATE, "spk_label_histogram: no pair rows (a loaded gamma table)");
    SPK_REQUIRE(n_pat >= 1 && 3 * n_pat <= ((int64_t)1 << 30), SPK_E_LIMIT,
                "spk_label_histogram: more than 2^30 (state, pattern) counters");
    Table &t0 = ctx->table[0], &t1 = ctx->side_table(1);
    SPK_REQUIRE(t0.n >= 0 && t1.n >= 0, SPK_E_STATE, "spk_label_histogram: no tables");
    const int64_t n0 = t0.n, n1 = t1.n;  // not link_only: t1 is t0, and ids_side1 (if given) describes its rows too
    // everything below lives for this call only
    LabelIds L;
    DevBuf<unsigned long long> hist;
    DevBuf<double> mpat;
    StageTimer T{ctx};
    SPK_TRY(hist.alloc((size_t)3 * n_pat));
    if (out_pattern_mp) SPK_TRY(mpat.alloc((size_t)n_pat));
    SPK_TRY(stage_label_ids(ctx, "spk_label_histogram", ids_side0, ids_side1, n0, n1, T, L));
    hipStream_t st = ctx->stream;
    unsigned int h_bad = 0u;
    // ---- mp per pattern (spk_score's own kernel and arguments) and the counts
    SPK_TRY(T.open());
    if (out_pattern_mp) SPK_TRY(pattern_mp_table(ctx, lambda, one_minus, m, u, mpat.p));
    SPK_HIP(hipMemsetAsync(hist.p, 0, (size_t)3 * n_pat * 8, st));
    if (P > 0) {
        LabelArgs A{};
        A.P = P;
        A.pl = ctx->pl.p;
        A.pr = ctx->pr.p;
        A.lab0 = L.side0();
        A.lab1 = L.side1();
        A.n0 = (uint32_t)n0;
        A.n1 = (uint32_t)n1;
        A.n_pat = (uint32_t)n_pat;
        A.ghist = hist.p;
        A.bad = L.bad.p;
        const bool lds = 3 * n_pat * 4 <= std::min<int64_t>(LH_LDS_BYTES, ctx->lds_per_block);
        if (ctx->code_bytes == 2) SPK_TRY(launch_label_hist<uint16_t>(ctx, A, lds));
        else SPK_TRY(launch_label_hist<uint32_t>(ctx, A, lds));
    }
    SPK_TRY(T.stop());  // the read-backs are no launches
    SPK_HIP(hipMemcpyAsync(&h_bad, L.bad.p, sizeof(h_bad), hipMemcpyDeviceToHost, st));
    SPK_HIP(hipMemcpyAsync(out_counts, hist.p, (size_t)3 * n_pat * 8, hipMemcpyDeviceToHost, st));
    if (out_pattern_mp) SPK_HIP(hipMemcpyAsync(out_pattern_mp, mpat.p, (size_t)n_pat * 8, hipMemcpyDeviceToHost, st));
    SPK_HIP(hipStreamSynchronize(st));
    SPK_TRY(T.add());
    SPK_REQUIRE(h_bad == 0u, SPK_E_STATE,
                "spk_label_histogram: a pair names a row outside its table or a code outside the pattern space");
    ctx->label_pairs = P;
    ctx->label_ms = T.result();
    return SPK_OK;
}

extern "C" int spk_label_info(spk_ctx *ctx, int64_t *out_pairs, double *out_ms) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "spk_label_info: null ctx");
    if (out_pairs) *out_pairs = ctx->label_pairs;
    if (out_ms) *out_ms = ctx->label_ms;
    return SPK_OK;
}

extern "C" int spk_label_scores_tf(spk_ctx *ctx, const int64_t *label_ids0, const int64_t *label_ids1, double lambda,
                                   double one_minus, const double *m, const double *u, int n_tf_cols,
                                   const int64_t *const *ids_side0, const int64_t *const *ids_side1,
                                   const double *const *adj_tables, const int64_t *table_sizes, int n_thresholds,
                                   const double *thresholds, uint64_t *out_counts) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "spk_label_scores_tf: null ctx");
    SPK_HIP(hipSetDevice(ctx->device));
    ctx->score_pairs = -1;
    ctx->score_ms = -1.0;
    ScoreCall C(ctx, "spk_label_scores_tf");
    SPK_TRY(scores_tf_begin(C, label_ids0, label_ids1, m, u, n_tf_cols, ids_side0 && ids_side1, adj_tables, table_sizes,
                            n_thresholds, thresholds, out_counts));
    TfStage G;  // the id arrays and tables live until this call returns
    SPK_TRY(tf_stage_host_ids(ctx, n_tf_cols, ids_side0, ids_side1, G));
    return scores_tf_run(C, G, label_ids0, label_ids1, lambda, one_minus, m, u, adj_tables, table_sizes, thresholds,
                         out_counts);
}

extern "C" int spk_label_scores_tf_columns(spk_ctx *ctx, const int64_t *label_ids0, const int64_t *label_ids1,
                                           double lambda, double one_minus, const double *m, const double *u,
                                           int n_tf_cols, const int32_t *cols, const double *const *adj_tables,
                                           const int64_t *table_sizes, int n_thresholds, const double *thresholds,
                                           uint64_t *out_counts) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "spk_label_scores_tf_columns: null ctx");
    SPK_HIP(hipSetDevice(ctx->device));
    ctx->score_pairs = -1;
    ctx->score_ms = -1.0;
    ScoreCall C(ctx, "spk_label_scores_tf_columns");
    SPK_TRY(scores_tf_begin(C, label_ids0, label_ids1, m, u, n_tf_cols, cols != nullptr, adj_tables, table_sizes,
                            n_thresholds, thresholds, out_counts));
    TfStage G;
    SPK_TRY(tf_stage_column_ids(ctx, n_tf_cols, cols, G));
    return scores_tf_run(C, G, label_ids0, label_ids1, lambda, one_minus, m, u, adj_tables, table_sizes, thresholds,
                         out_counts);
}

extern "C" int spk_label_scores_selection(spk_ctx *ctx, const int64_t *label_ids0, const int64_t *label_ids1, int field,
                                          int n_thresholds, const double *thresholds, uint64_t *out_counts) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "spk_label_scores_selection: null ctx");
    SPK_HIP(hipSetDevice(ctx->device));
    ctx->score_pairs = -1;
    ctx->score_ms = -1.0;
    ScoreCall C(ctx, "spk_label_scores_selection");
    SPK_TRY(C.check(label_ids0, label_ids1, n_thresholds, thresholds, out_counts));
    SPK_REQUIRE(field == SPK_SEL_MP || field == SPK_SEL_TF_MP, SPK_E_INVALID,
                "spk_label_scores_selection: unknown field");
    const Selection &S = ctx->sel;
    SPK_REQUIRE(S.valid, SPK_E_STATE, "spk_label_scores_selection: no selection (run spk_select*)");
    SPK_REQUIRE(S.current(ctx), SPK_E_STATE,
                "spk_label_scores_selection: the pairs or codes changed since spk_select*");
    SPK_REQUIRE(S.has_rows, SPK_E_STATE, "spk_label_scores_selection: no pair rows (a loaded gamma table)");
    SPK_REQUIRE(field != SPK_SEL_MP || S.has_mp, SPK_E_STATE, "spk_label_scores_selection: spk_select got no m / u");
    SPK_REQUIRE(field != SPK_SEL_TF_MP || S.has_tf, SPK_E_STATE,
                "spk_label_scores_selection: the selection was made without tf tables (spk_select)");
    SPK_REQUIRE(ctx->n_patterns >= 1 && ctx->n_patterns <= (int64_t)UINT32_MAX, SPK_E_LIMIT,
                "spk_label_scores_selection: pattern space");
    const int64_t n = S.n, n0 = ctx->table[0].n, n1 = ctx->side_table(1).n;
    SPK_REQUIRE(n0 >= 0 && n1 >= 0, SPK_E_STATE, "spk_label_scores_selection: no tables");
    hipStream_t st = ctx->stream;
    SPK_TRY(C.stage(label_ids0, label_ids1, thresholds, n0, n1));
    SPK_TRY(C.timer.open());
    SPK_HIP(hipMemsetAsync(C.cnt.p, 0, (size_t)3 * (C.T + 2) * 8, st));
    if (n > 0) {
        ScoreArgs A{};
        C.fill(A, n, S.l.p, S.r.p, n0, n1);
        A.code = S.code.p;
        A.mpat = S.mpat.p;
        A.per_pair = field == SPK_SEL_TF_MP ? S.tf_mp.p : nullptr;
        k_label_scores_sel<<<score_grid(ctx, n, 1, LS_SEL_WG_PER_CU), LS_THREADS, score_lds_bytes(C.T), st>>>(A);
        SPK_HIP(hipGetLastError());
    }
    return C.finish(n, out_counts);
}

extern "C" int spk_label_pairs_histogram(spk_ctx *ctx, int64_t n_labels, const int32_t *rows_l, const int32_t *rows_r,
                                         const uint8_t *is_match, double lambda, double one_minus, const double *m,
                                         const double *u, uint64_t *out_counts, double *out_pattern_mp,
                                         int32_t *out_label_code) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "spk_label_pairs_histogram: null ctx");
    SPK_HIP(hipSetDevice(ctx->device));
    ctx->lpairs_pairs = ctx->lpairs_capacity = -1;
    ctx->lpairs_ms = -1.0;
    ctx->lpairs_max_probe = -1;
    SPK_REQUIRE(n_labels >= 0, SPK_E_INVALID, "spk_label_pairs_histogram: negative n_labels");
    SPK_REQUIRE(n_labels == 0 || (rows_l && rows_r && is_match), SPK_E_INVALID,
                "spk_label_pairs_histogram: null rows_l, rows_r or is_match");
    SPK_REQUIRE(out_counts, SPK_E_INVALID, "spk_label_pairs_histogram: null out_counts");
    SPK_REQUIRE((m == nullptr) == (u == nullptr), SPK_E_INVALID, "spk_label_pairs_histogram: m and u come together");
    SPK_REQUIRE(!out_pattern_mp || (m && u), SPK_E_INVALID, "spk_label_pairs_histogram: out_pattern_mp needs m and u");
    SPK_REQUIRE(ctx->codes_valid, SPK_E_STATE, "spk_label_pairs_histogram: no gammas");
    SPK_TRY(settle_gammas(ctx, nullptr));
    SPK_REQUIRE(ctx->codes_valid, SPK_E_STATE, "spk_label_pairs_histogram: no gammas");
    const int64_t P = ctx->n_pairs, n_pat = ctx->n_patterns;
    SPK_REQUIRE(ctx->pairs_valid && ctx->pl.p && ctx->pr.p && ctx->pl.n >= (size_t)P && ctx->pr.n >= (size_t)P,
                SPK_E_STATE, "spk_label_pairs_histogram: no pair rows (a loaded gamma table)");
    SPK_REQUIRE(n_labels <= LP_MAX_LABELS, SPK_E_LIMIT, "spk_label_pairs_histogram: more than 2^27 labelled pairs");
    SPK_REQUIRE(n_pat >= 1 && 3 * n_pat <= ((int64_t)1 << 30), SPK_E_LIMIT,
                "spk_label_pairs_histogram: more than 2^30 (state, pattern) counters");
    Table &t0 = ctx->table[0], &t1 = ctx->side_table(1);
    SPK_REQUIRE(t0.n >= 0 && t1.n >= 0, SPK_E_STATE, "spk_label_pairs_histogram: no tables");
    // everything below lives for this call only
    PairTableStage S;
    DevBuf<unsigned long long> hist;
    DevBuf<int32_t> code;
    DevBuf<double> mpat;
    StageTimer T{ctx};
    SPK_TRY(hist.alloc((size_t)3 * n_pat));
    if (out_pattern_mp) SPK_TRY(mpat.alloc((size_t)n_pat));
    if (out_label_code && n_labels > 0) SPK_TRY(code.alloc((size_t)n_labels));
    hipStream_t st = ctx->stream;
    SPK_TRY(stage_pair_table(ctx, "spk_label_pairs_histogram", n_labels, rows_l, rows_r, is_match, t0.n, t1.n, T, S));
    const int64_t capacity = S.capacity;
    unsigned int h_flags[2] = {0u, (unsigned int)S.max_probe};
    DevBuf<unsigned int> &flags = S.flags;
    // ---- mp per pattern (spk_score's own kernel and arguments) and the counts
    SPK_TRY(T.open());
    if (code.p) SPK_HIP(hipMemsetAsync(code.p, 0xFF, (size_t)n_labels * 4, st));  // -1
    if (out_pattern_mp) SPK_TRY(pattern_mp_table(ctx, lambda, one_minus, m, u, mpat.p));
    SPK_HIP(hipMemsetAsync(hist.p, 0, (size_t)3 * n_pat * 8, st));
    if (P > 0) {
        PairLabelArgs A{};
        A.P = P;
        A.pl = ctx->pl.p;
        A.pr = ctx->pr.p;
        A.T = S.tab;
        A.n0 = (uint32_t)t0.n;
        A.n1 = (uint32_t)t1.n;
        A.n_pat = (uint32_t)n_pat;
        A.label_code = code.p;
        A.ghist = hist.p;
        A.bad = flags.p;
        const bool lds = 3 * n_pat * 4 <= std::min<int64_t>(LH_LDS_BYTES, ctx->lds_per_block);
        if (ctx->code_bytes == 2) SPK_TRY(launch_label_pairs_hist<uint16_t>(ctx, A, lds));
        else SPK_TRY(launch_label_pairs_hist<uint32_t>(ctx, A, lds));
    }
    SPK_TRY(T.stop());  // the read-backs are no launches
    unsigned int h_bad = 0u;
    SPK_HIP(hipMemcpyAsync(&h_bad, flags.p, sizeof(h_bad), hipMemcpyDeviceToHost, st));
    SPK_HIP(hipMemcpyAsync(out_counts, hist.p, (size_t)3 * n_pat * 8, hipMemcpyDeviceToHost, st));
    if (out_pattern_mp) SPK_HIP(hipMemcpyAsync(out_pattern_mp, mpat.p, (size_t)n_pat * 8, hipMemcpyDeviceToHost, st));
    if (out_label_code && n_labels > 0)
        SPK_HIP(hipMemcpyAsync(out_label_code, code.p, (size_t)n_labels * 4, hipMemcpyDeviceToHost, st));
    SPK_HIP(hipStreamSynchronize(st));
    SPK_TRY(T.add());
    SPK_REQUIRE(!(h_bad & LP_BAD_PAIR), SPK_E_STATE,
                "spk_label_pairs_histogram: a pair names a row outside its table or a code outside the pattern space");
    SPK_REQUIRE(h_bad == 0u, SPK_E_STATE, "spk_label_pairs_histogram: the pair table is damaged");
    ctx->lpairs_pairs = P;
    ctx->lpairs_ms = T.result();
    ctx->lpairs_capacity = capacity;
    ctx->lpairs_max_probe = (int)h_flags[1];
    return SPK_OK;
}

extern "C" int spk_label_pairs_info(spk_ctx *ctx, int64_t *out_pairs, double *out_ms, int64_t *out_capacity,
                                    int *out_max_probe) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "spk_label_pairs_info: null ctx");
    if (out_pairs) *out_pairs = ctx->lpairs_pairs;
    if (out_ms) *out_ms = ctx->lpairs_ms;
    if (out_capacity) *out_capacity = ctx->lpairs_capacity;
    if (out_max_probe) *out_max_probe = ctx->lpairs_max_probe;
    return SPK_OK;
}

static void pair_scores_info_reset(spk_ctx *ctx) {
    ctx->lpscore_pairs = ctx->lpscore_capacity = -1;
    ctx->lpscore_ms = -1.0;
    ctx->lpscore_max_probe = -1;
}

extern "C" int spk_label_pairs_scores_tf(spk_ctx *ctx, int64_t n_labels, const int32_t *rows_l, const int32_t *rows_r,
                                         const uint8_t *is_match, double lambda, double one_minus, const double *m,
                                         const double *u, int n_tf_cols, const int64_t *const *ids_side0,
                                         const int64_t *const *ids_side1, const double *const *adj_tables,
                                         const int64_t *table_sizes, int n_thresholds, const double *thresholds,
                                         uint64_t *out_counts, int64_t *out_label_pair, double *out_label_score) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "spk_label_pairs_scores_tf: null ctx");
    SPK_HIP(hipSetDevice(ctx->device));
    pair_scores_info_reset(ctx);
    PairScoreCall C(ctx, "spk_label_pairs_scores_tf");
    SPK_TRY(pair_scores_tf_begin(C, n_labels, rows_l, rows_r, is_match, m, u, n_tf_cols, ids_side0 && ids_side1,
                                 adj_tables, table_sizes, n_thresholds, thresholds, out_counts, out_label_pair,
                                 out_label_score));
    TfStage G;  // the id arrays and tables live until this call returns
    SPK_TRY(tf_stage_host_ids(ctx, n_tf_cols, ids_side0, ids_side1, G));
    return pair_scores_tf_run(C, G, rows_l, rows_r, is_match, lambda, one_minus, m, u, adj_tables, table_sizes,
                              thresholds, out_counts, out_label_pair, out_label_score);
}

extern "C" int spk_label_pairs_scores_tf_columns(spk_ctx *ctx, int64_t n_labels, const int32_t *rows_l,
                                                 const int32_t *rows_r, const uint8_t *is_match, double lambda,
                                                 double one_minus, const double *m, const double *u, int n_tf_cols,
                                                 const int32_t *cols, const double *const *adj_tables,
                                                 const int64_t *table_sizes, int n_thresholds, const double *thresholds,
                                                 uint64_t *out_counts, int64_t *out_label_pair,
                                                 double *out_label_score) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "spk_label_pairs_scores_tf_columns: null ctx");
    SPK_HIP(hipSetDevice(ctx->device));
    pair_scores_info_reset(ctx);
    PairScoreCall C(ctx, "spk_label_pairs_scores_tf_columns");
    SPK_TRY(pair_scores_tf_begin(C, n_labels, rows_l, rows_r, is_match, m, u, n_tf_cols, cols != nullptr, adj_tables,
                                 table_sizes, n_thresholds, thresholds, out_counts, out_label_pair, out_label_score));
    TfStage G;
    SPK_TRY(tf_stage_column_ids(ctx, n_tf_cols, cols, G));
    return pair_scores_tf_run(C, G, rows_l, rows_r, is_match, lambda, one_minus, m, u, adj_tables, table_sizes,
                              thresholds, out_counts, out_label_pair, out_label_score);
}

extern "C" int spk_label_pairs_scores_selection(spk_ctx *ctx, int64_t n_labels, const int32_t *rows_l,
                                                const int32_t *rows_r, const uint8_t *is_match, int field,
                                                int n_thresholds, const double *thresholds, uint64_t *out_counts,
                                                int64_t *out_label_pair, double *out_label_score) {
    const char *what = "spk_label_pairs_scores_selection";
    SPK_REQUIRE(ctx, SPK_E_INVALID, "spk_label_pairs_scores_selection: null ctx");
    SPK_HIP(hipSetDevice(ctx->device));
    pair_scores_info_reset(ctx);
    PairScoreCall C(ctx, what);
    const std::string w(what);
    SPK_TRY(C.check(n_labels, rows_l, rows_r, is_match, n_thresholds, thresholds, out_counts, out_label_pair,
                    out_label_score));
    SPK_REQUIRE(field == SPK_SEL_MP || field == SPK_SEL_TF_MP, SPK_E_INVALID, w + ": unknown field");
    const Selection &S = ctx->sel;
    SPK_REQUIRE(S.valid, SPK_E_STATE, w + ": no selection (run spk_select*)");
    SPK_REQUIRE(S.current(ctx), SPK_E_STATE, w + ": the pairs or codes changed since spk_select*");
    SPK_REQUIRE(S.has_rows, SPK_E_STATE, w + ": no pair rows (a loaded gamma table)");
    SPK_REQUIRE(field != SPK_SEL_MP || S.has_mp, SPK_E_STATE, w + ": spk_select got no m / u");
    SPK_REQUIRE(field != SPK_SEL_TF_MP || S.has_tf, SPK_E_STATE,
                w + ": the selection was made without tf tables (spk_select)");
    SPK_REQUIRE(ctx->n_patterns >= 1 && ctx->n_patterns <= (int64_t)UINT32_MAX, SPK_E_LIMIT, w + ": pattern space");
    const int64_t n = S.n, n0 = ctx->table[0].n, n1 = ctx->side_table(1).n;
    SPK_REQUIRE(n0 >= 0 && n1 >= 0, SPK_E_STATE, w + ": no tables");
    hipStream_t st = ctx->stream;
    SPK_TRY(C.stage(rows_l, rows_r, is_match, thresholds, n0, n1));
    SPK_TRY(C.timer.open());
    SPK_TRY(C.clear());
    PairScoreArgs B{};
    C.fill(B, n, S.l.p, S.r.p, n0, n1);
    B.S.code = S.code.p;
    B.S.mpat = S.mpat.p;
    B.S.per_pair = field == SPK_SEL_TF_MP ? S.tf_mp.p : nullptr;
    if (n > 0) {
        k_label_pairs_scores_sel<<<score_grid(ctx, n, 1, LPS_SEL_WG_PER_CU), LS_THREADS, score_lds_bytes(C.T), st>>>(B);
        SPK_HIP(hipGetLastError());
    }
    SPK_TRY(C.per_label_launch<uint32_t>(B, false, TfApply{}, S.code.p));
    return C.finish(n, out_counts, out_label_pair, out_label_score);
}

extern "C" int spk_label_pairs_scores_info(spk_ctx *ctx, int64_t *out_pairs, double *out_ms, int64_t *out_capacity,
                                           int *out_max_probe) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "spk_label_pairs_scores_info: null ctx");
    if (out_pairs) *out_pairs = ctx->lpscore_pairs;
    if (out_ms) *out_ms = ctx->lpscore_ms;
    if (out_capacity) *out_capacity = ctx->lpscore_capacity;
    if (out_max_probe) *out_max_probe = ctx->lpscore_max_probe;
    return SPK_OK;
}

extern "C" int spk_label_scores_info(spk_ctx *ctx, int64_t *out_pairs, double *out_ms) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "spk_label_scores_info: null ctx");
    if (out_pairs) *out_pairs = ctx->score_pairs;
    if (out_ms) *out_ms = ctx->score_ms;
    return SPK_OK;
}
