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
static unsigned label_grid(const spk_ctx *ctx, int64_t P) {
    const int64_t steps = (P / LH_PAIRS + LH_THREADS - 1) / LH_THREADS;
    int64_t g = std::min<int64_t>(steps, LH_WG_PER_CU * (int64_t)ctx->n_cu);
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
    hipStream_t st = ctx->stream;
    // everything below lives for this call only
    DevBuf<int64_t> wide;
    DevBuf<int32_t> lab0, lab1;
    DevBuf<unsigned long long> hist;
    DevBuf<double> mpat;
    DevBuf<unsigned int> bad;
    const bool second = ids_side1 && (two || ids_side1 != ids_side0);  // the right rows have an id array of their own
    SPK_TRY(wide.alloc((size_t)std::max(n0, second ? n1 : 0) + 1));
    SPK_TRY(lab0.alloc((size_t)n0 + 1));
    if (second) SPK_TRY(lab1.alloc((size_t)n1 + 1));
    SPK_TRY(hist.alloc((size_t)3 * n_pat));
    SPK_TRY(bad.alloc(1));
    if (out_pattern_mp) SPK_TRY(mpat.alloc((size_t)n_pat));
    SPK_HIP(hipMemsetAsync(bad.p, 0, sizeof(unsigned int), st));
    StageTimer T{ctx};
    // ---- the label ids, narrowed to 32 bits on the device (the upload itself is not a launch: outside the interval)
    auto narrow = [&](const int64_t *ids, int64_t n, int32_t *out) -> int {
        if (n == 0) return SPK_OK;
        SPK_HIP(hipMemcpyAsync(wide.p, ids, (size_t)n * 8, hipMemcpyHostToDevice, st));
        SPK_TRY(T.open());
        k_label_narrow<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(n, wide.p, out, bad.p);
        SPK_HIP(hipGetLastError());
        return T.close();  // synchronises: the next upload reuses `wide`; the source is borrowed for the call
    };
    SPK_TRY(narrow(ids_side0, n0, lab0.p));
    if (second) SPK_TRY(narrow(ids_side1, n1, lab1.p));
    unsigned int h_bad = 0u;
    SPK_HIP(hipMemcpyAsync(&h_bad, bad.p, sizeof(h_bad), hipMemcpyDeviceToHost, st));
    SPK_HIP(hipStreamSynchronize(st));
    SPK_REQUIRE(h_bad == 0u, SPK_E_INVALID, "spk_label_histogram: a label id of 2^31 or more");
    // ---- mp per pattern (spk_score's own kernel and arguments) and the counts
    SPK_TRY(T.open());
    if (out_pattern_mp) SPK_TRY(pattern_mp_table(ctx, lambda, one_minus, m, u, mpat.p));
    SPK_HIP(hipMemsetAsync(hist.p, 0, (size_t)3 * n_pat * 8, st));
    if (P > 0) {
        LabelArgs A{};
        A.P = P;
        A.pl = ctx->pl.p;
        A.pr = ctx->pr.p;
        A.lab0 = lab0.p;
        A.lab1 = second ? lab1.p : lab0.p;
        A.n0 = (uint32_t)n0;
        A.n1 = (uint32_t)n1;
        A.n_pat = (uint32_t)n_pat;
        A.ghist = hist.p;
        A.bad = bad.p;
        const bool lds = 3 * n_pat * 4 <= std::min<int64_t>(LH_LDS_BYTES, ctx->lds_per_block);
        if (ctx->code_bytes == 2) SPK_TRY(launch_label_hist<uint16_t>(ctx, A, lds));
        else SPK_TRY(launch_label_hist<uint32_t>(ctx, A, lds));
    }
    SPK_TRY(T.stop());  // the read-backs are no launches
    SPK_HIP(hipMemcpyAsync(&h_bad, bad.p, sizeof(h_bad), hipMemcpyDeviceToHost, st));
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
