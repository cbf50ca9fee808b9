// Random record pairs drawn on the device (spk_pairs_sample; the definition of a draw is in include/splink_hip.h).
//
// A draw is a pure function of its ordinal, so the launch shape is free: a workgroup takes SM_CHUNK consecutive
// ordinals, a thread SM_PER_THREAD consecutive ones of them.  Consecutive ordinals have consecutive (stratified)
// anchors, so the anchor-side rank reads of a thread are a short run and those of a wave a contiguous stretch; the
// partner's rank is the one gathered 8-byte read per draw.  Dedupe draws can be dropped (equal ranks, NULL unique
// ids), so they go through the count / scan / emit form of k_enum (spk_block.hip): the survivors per chunk are
// counted, the counts scanned, and the emit pass compacts a workgroup's survivors in LDS and stores them with
// consecutive lanes on consecutive positions, in ordinal order.  Every link_only draw survives: no count pass, a
// chunk's pairs start at its first ordinal.
#include <algorithm>

#include "spk_internal.h"
#include "spk_prim.h"

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "spk_sample.hip targets gfx950 (MI355X) only"
#endif

namespace spk {

static constexpr int SM_THREADS = 256;
static constexpr int SM_PER_THREAD = 8;
static constexpr int64_t SM_CHUNK = (int64_t)SM_THREADS * SM_PER_THREAD;
static constexpr int SM_WAVES = SM_THREADS / 64;

__host__ __device__ inline uint64_t sm_mix(uint64_t x) {
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

__device__ inline uint64_t sm_word(uint64_t seed_mix, uint64_t i, uint64_t j) {
    return sm_mix(seed_mix + 0x9E3779B97F4A7C15ull * (3ull * i + j + 1ull));
}

struct SampleArgs {
    uint64_t seed_mix;         // mix(seed)
    uint64_t total;            // total_draws (> 0)
    uint64_t step_q, step_r;   // n0 / total, n0 % total: the anchor slice bounds advance by these per ordinal
    int64_t q0, q1;            // the ordinals of this call
    uint64_t n0, n1;
    const int64_t *rank;       // table 0's ranks, or null (link_only: every draw survives)
    int64_t null_div;
    int64_t *chunk_count;      // count pass output
    const int64_t *chunk_off;  // emit pass input, or null (link_only: chunk c starts at c * SM_CHUNK)
    int32_t *out_l, *out_r;
};

template <bool EMIT>
__global__ __launch_bounds__(SM_THREADS) void k_sample(SampleArgs A) {
    __shared__ int s_wave[SM_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t base = A.q0 + (int64_t)blockIdx.x * SM_CHUNK + (int64_t)threadIdx.x * SM_PER_THREAD;
    int32_t xs[SM_PER_THREAD], ys[SM_PER_THREAD];
    unsigned keep = 0;
    if (base < A.q1) {
        // lo = (i * n0) / total and its remainder for the thread's first ordinal (total * n0 < 2^63: no overflow);
        // the next slice bound follows from n0 = step_q * total + step_r without another division
        const uint64_t p = (uint64_t)base * A.n0;
        uint64_t lo = p / A.total, rem = p - lo * A.total;
#pragma unroll
        for (int k = 0; k < SM_PER_THREAD; ++k) {
            const uint64_t i = (uint64_t)base + (uint64_t)k;
            uint64_t hi = lo + A.step_q, hrem = rem + A.step_r;
            if (hrem >= A.total) {
                hrem -= A.total;
                ++hi;
            }
            if ((int64_t)i < A.q1) {
                const uint64_t a = hi > lo ? lo + __umul64hi(sm_word(A.seed_mix, i, 0), hi - lo) : lo;
                const uint64_t w1 = sm_word(A.seed_mix, i, 1);
                bool ok = true;
                uint64_t l = a, r;
                if (!A.rank) {
                    r = __umul64hi(w1, A.n1);
                } else {
                    uint64_t b = __umul64hi(w1, A.n0 - 1);
                    b += b >= a ? 1u : 0u;
                    const int64_t ra = A.rank[a], rb = A.rank[b];
                    ok = ra != rb;
                    // the NULL-unique-id rule of k_enum (spk_block.hip)
                    if (ok && A.null_div > 0 && ra / A.null_div == rb / A.null_div &&
                        (ra % A.null_div == A.null_div - 1 || rb % A.null_div == A.null_div - 1))
                        ok = false;
                    l = ra < rb ? a : b;
                    r = ra < rb ? b : a;
                }
                xs[k] = (int32_t)l;
                ys[k] = (int32_t)r;
                if (ok) keep |= 1u << k;
            }
            lo = hi;
            rem = hrem;
        }
    }
    // exclusive prefix of the per-thread counts over the workgroup: shuffles inside a wave, the waves' totals in LDS
    const int cnt = __popc(keep);
    int incl = cnt;
    for (int off = 1; off < 64; off <<= 1) {
        const int v = __shfl_up(incl, off, 64);
        if (lane >= off) incl += v;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < SM_WAVES; ++w) {
        const int c = s_wave[w];
        before += w < wave ? c : 0;
        total += c;
    }
    if (!EMIT) {
        if (threadIdx.x == 0) A.chunk_count[blockIdx.x] = total;
        return;
    }
    __shared__ int32_t s_out[2][SM_CHUNK];
    int loc = before + incl - cnt;
#pragma unroll
    for (int k = 0; k < SM_PER_THREAD; ++k) {
        if (keep & (1u << k)) {
            s_out[0][loc] = xs[k];
            s_out[1][loc] = ys[k];
            ++loc;
        }
    }
    __syncthreads();
    const int64_t out0 = A.chunk_off ? A.chunk_off[blockIdx.x] : (int64_t)blockIdx.x * SM_CHUNK;
    for (int k = threadIdx.x; k < total; k += SM_THREADS) {
        A.out_l[out0 + k] = s_out[0][k];
        A.out_r[out0 + k] = s_out[1][k];
    }
}

}  // namespace spk

using namespace spk;

namespace {
// Until the sampled set is in place, a failure leaves no pair set.
struct SampleCommit {
    spk_ctx *ctx;
    bool done = false;
    ~SampleCommit() {
        if (!done) ctx->pairs_dropped();
    }
};
}  // namespace

extern "C" int spk_pairs_sample(spk_ctx *ctx, int link_type, uint64_t seed, int64_t total_draws, int64_t first_draw,
                                int64_t n_draws, int64_t *out_n_pairs) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "spk_pairs_sample: null ctx");
    ctx->pairs_dropped();
    SampleCommit commit{ctx};
    ctx->sample_draws = ctx->sample_kept = -1;
    ctx->sample_ms = -1.0;
    SPK_REQUIRE(link_type >= 0 && link_type <= 2, SPK_E_INVALID, "spk_pairs_sample: bad link_type");
    SPK_REQUIRE(total_draws >= 0 && first_draw >= 0 && n_draws >= 0 && first_draw <= total_draws &&
                    n_draws <= total_draws - first_draw,
                SPK_E_INVALID, "spk_pairs_sample: the range must lie in [0, total_draws)");
    SPK_HIP(hipSetDevice(ctx->device));
    const bool link_only = link_type == SPK_LINK_ONLY;
    Table &tl = ctx->table[0];
    Table &tr = ctx->table[link_only ? 1 : 0];
    SPK_REQUIRE(tl.n >= 0 && tr.n >= 0, SPK_E_STATE, "spk_pairs_sample: tables not loaded");
    SPK_REQUIRE(link_only || tl.rank.p || tl.n == 0, SPK_E_STATE, "spk_pairs_sample: rank not set");
    SPK_REQUIRE((__int128)total_draws * (__int128)tl.n < ((__int128)1 << 63), SPK_E_LIMIT,
                "spk_pairs_sample: total_draws x rows of table 0 must fit in 63 bits");
    SPK_REQUIRE(n_draws < (int64_t)1 << 40, SPK_E_LIMIT, "spk_pairs_sample: at most 2^40 draws per call");
    ctx->link_type = link_type;
    const int64_t n0 = tl.n, n1 = tr.n;
    const bool none = link_only ? (n0 == 0 || n1 == 0) : n0 < 2;
    const int64_t draws = none ? 0 : n_draws;
    const int64_t chunks = (draws + SM_CHUNK - 1) / SM_CHUNK;
    hipStream_t st = ctx->stream;
    StageTimer T{ctx};
    SampleArgs A{};
    int64_t n_out = 0;
    CountScan counts;
    DevBuf<uint8_t> tmp;
    if (draws > 0) {
        A.seed_mix = sm_mix(seed);
        A.total = (uint64_t)total_draws;
        A.step_q = (uint64_t)n0 / A.total;
        A.step_r = (uint64_t)n0 % A.total;
        A.q0 = first_draw;
        A.q1 = first_draw + draws;
        A.n0 = (uint64_t)n0;
        A.n1 = (uint64_t)n1;
        A.rank = link_only ? nullptr : tl.rank.p;
        A.null_div = link_only ? 0 : tl.null_div;
        n_out = draws;
        if (!link_only) {
            SPK_TRY(counts.alloc(ctx, chunks));
            A.chunk_count = counts.count.p;
            SPK_TRY(T.open());
            k_sample<false><<<(unsigned)chunks, SM_THREADS, 0, st>>>(A);
            SPK_HIP(hipGetLastError());
            SPK_TRY(scan_total(ctx, counts, tmp, &T));
            n_out = counts.total;
            SPK_REQUIRE(n_out >= 0 && n_out <= draws, SPK_E_STATE, "spk_pairs_sample: survivor count");
            A.chunk_count = nullptr;
            A.chunk_off = counts.off.p;
        }
    }
    SPK_TRY(ctx->pl.alloc((size_t)n_out + 1));
    SPK_TRY(ctx->pr.alloc((size_t)n_out + 1));
    if (draws > 0) {
        A.out_l = ctx->pl.p;
        A.out_r = ctx->pr.p;
        SPK_TRY(T.open());
        k_sample<true><<<(unsigned)chunks, SM_THREADS, 0, st>>>(A);
        SPK_HIP(hipGetLastError());
    }
    SPK_TRY(T.close());  // synchronises, draws or none
    ctx->pairs_replaced(n_out);
    ctx->pair_terms.clear();  // as a loaded list: no rules, so no key terms, no rule ranges, no views
    ctx->set_rule_ranges({}, n_out);
    commit.done = true;
    ctx->sample_draws = n_draws;
    ctx->sample_kept = n_out;
    ctx->sample_ms = T.result();
    if (out_n_pairs) *out_n_pairs = n_out;
    return SPK_OK;
}

extern "C" int spk_pairs_sample_info(spk_ctx *ctx, int64_t *out_draws, int64_t *out_kept, double *out_ms) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "spk_pairs_sample_info: null ctx");
    if (out_draws) *out_draws = ctx->sample_draws;
    if (out_kept) *out_kept = ctx->sample_kept;
    if (out_ms) *out_ms = ctx->sample_ms;
    return SPK_OK;
}
