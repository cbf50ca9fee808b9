// The jar's UDFs as bulk device functions (JaroWinklerSimilarity.call, Spark levenshtein,
// JaccardSimilarity.call, CosineDistance.call): spk_jaro_winkler_sim, spk_levenshtein, spk_jaccard_sim
// and spk_cosine_distance.
// Same device code as the comparison passes: LDS-staged jw_small / lev_myers / jaccard_units /
// cosine_tokens for short strings, the global-memory forms for the rest, and pairs with a string past
// SLOW_LIMIT units through the huge pass (device scratch sized to the longest string).
#include <algorithm>

#include "spk_gamma.h"

using namespace spk;

struct UdfArgs {
    int64_t n;
    const uint16_t *u16;
    const int64_t *off;  // [2n+1]: string i of pair p is 2p (left) and 2p+1 (right)
    const int32_t *cp;   // code points per string
    int op;              // 0 JW, 1 Levenshtein, 2 jaccard_sim, 3 cosine_distance
    double *out;
    int32_t *huge;              // pairs for k_udf_huge
    unsigned int *n_huge;
};

__device__ inline StrView udf_view(const UdfArgs &U, int64_t s) {
    return plain_view(U.u16 + U.off[s], (int32_t)(U.off[s + 1] - U.off[s]), U.cp[s]);
}

__global__ __launch_bounds__(U_THREADS) void k_udf(UdfArgs U) {
    __shared__ uint16_t lds[2][MAXU][U_THREADS];
    uint16_t *slot_a = &lds[0][0][threadIdx.x];
    uint16_t *slot_b = &lds[1][0][threadIdx.x];
    int64_t p = (int64_t)blockIdx.x * U_THREADS + threadIdx.x;
    if (p >= U.n) return;
    const StrView a = udf_view(U, 2 * p), b = udf_view(U, 2 * p + 1);
    if (a.n > SLOW_LIMIT || b.n > SLOW_LIMIT) {
        U.huge[atomicAdd(U.n_huge, 1u)] = (int32_t)p;
        return;
    }
    if (U.op == 0) {
        double v;
        if (a.n <= MAXU && b.n <= MAXU) {
            stage<U_THREADS>(slot_a, a);
            stage<U_THREADS>(slot_b, b);
            v = jw_small(LdsAcc<U_THREADS>{slot_a}, a.n, LdsAcc<U_THREADS>{slot_b}, b.n);
        } else {
            v = jw_long(GlbAcc{a.p}, a.n, GlbAcc{b.p}, b.n);
        }
        U.out[p] = v;
    } else {
        int v;
        if (a.n <= MAXU && b.n <= MAXU && a.ncp == a.n && b.ncp == b.n) {
            stage<U_THREADS>(slot_a, a);
            stage<U_THREADS>(slot_b, b);
            v = lev_myers(LdsAcc<U_THREADS>{slot_a}, a.n, LdsAcc<U_THREADS>{slot_b}, b.n);
        } else {
            v = lev_long(a, b);
        }
        U.out[p] = (double)v;
    }
}

__global__ __launch_bounds__(64) void k_udf_huge(UdfArgs U, int64_t n, Scratch S) {
    S.slot = (int64_t)blockIdx.x * 64 + threadIdx.x;
    for (int64_t i = S.slot; i < n; i += S.n_slots) {
        const int64_t p = U.huge[i];
        const StrView a = udf_view(U, 2 * p), b = udf_view(U, 2 * p + 1);
        U.out[p] = U.op == 0 ? jw_long(GlbAcc{a.p}, a.n, GlbAcc{b.p}, b.n, S.at<uint64_t>(0), S.at<uint64_t>(S.words))
                             : (double)lev_long(a, b, S.at<uint32_t>(0), S.at<int32_t>(S.units));
    }
}

// Ops 2 and 3 (jaccard_sim, cosine_distance) as kernels of their own, so k_udf / k_udf_huge keep their register
// budget: the same three length classes.
__global__ __launch_bounds__(U_THREADS) void k_udf_set(UdfArgs U) {
    __shared__ uint16_t lds[2][MAXU][U_THREADS];
    uint16_t *slot_a = &lds[0][0][threadIdx.x];
    uint16_t *slot_b = &lds[1][0][threadIdx.x];
    int64_t p = (int64_t)blockIdx.x * U_THREADS + threadIdx.x;
    if (p >= U.n) return;
    const StrView a = udf_view(U, 2 * p), b = udf_view(U, 2 * p + 1);
    if (a.n > SLOW_LIMIT || b.n > SLOW_LIMIT) {
        U.huge[atomicAdd(U.n_huge, 1u)] = (int32_t)p;
        return;
    }
    const bool jac = U.op == 2;
    double v;
    if (a.n <= MAXU && b.n <= MAXU) {
        stage<U_THREADS>(slot_a, a);
        stage<U_THREADS>(slot_b, b);
        const LdsAcc<U_THREADS> la{slot_a}, lb{slot_b};
        v = jac ? jaccard_units(la, a.n, lb, b.n) : cosine_tokens(la, a.n, lb, b.n);
    } else {
        const GlbAcc ga{a.p}, gb{b.p};
        v = jac ? jaccard_units(ga, a.n, gb, b.n) : cosine_tokens(ga, a.n, gb, b.n);
    }
    U.out[p] = v;
}

__global__ __launch_bounds__(64) void k_udf_set_huge(UdfArgs U, int64_t n, Scratch S) {
    S.slot = (int64_t)blockIdx.x * 64 + threadIdx.x;
    for (int64_t i = S.slot; i < n; i += S.n_slots) {
        const int64_t p = U.huge[i];
        const StrView a = udf_view(U, 2 * p), b = udf_view(U, 2 * p + 1);
        const GlbAcc ga{a.p}, gb{b.p};
        U.out[p] = U.op == 2 ? jaccard_bitmap(ga, a.n, gb, b.n, S.at<uint64_t>(0), S.at<uint64_t>(JACCARD_WORDS))
                             : cosine_tokens(ga, a.n, gb, b.n);
    }
}

static int run_udf(spk_ctx *ctx, int op, int64_t n, const int64_t *l_off, const uint8_t *l_utf8, const int64_t *r_off,
                   const uint8_t *r_utf8, double *out) {
    SPK_REQUIRE(ctx && n >= 0 && out && l_off && r_off, SPK_E_INVALID, "spk udf: bad args");
    SPK_HIP(hipSetDevice(ctx->device));
    std::vector<uint16_t> u;
    std::vector<int64_t> off{0};
    std::vector<int32_t> cp;
    for (int64_t i = 0; i < n; ++i) {
        for (int side = 0; side < 2; ++side) {
            const int64_t *o = side ? r_off : l_off;
            const uint8_t *d = side ? r_utf8 : l_utf8;
            int32_t ncp = 0;
            auto v = utf8_to_utf16(d + o[i], o[i + 1] - o[i], &ncp);
            u.insert(u.end(), v.begin(), v.end());
            off.push_back((int64_t)u.size());
            cp.push_back(ncp);
        }
    }
    u.push_back(0);
    DevBuf<uint16_t> d_u;
    DevBuf<int64_t> d_off;
    DevBuf<int32_t> d_cp;
    DevBuf<double> d_out;
    DevBuf<int32_t> d_huge;
    DevBuf<unsigned int> d_nhuge;
    SPK_TRY(d_u.alloc(u.size()));
    SPK_TRY(d_off.alloc(off.size()));
    SPK_TRY(d_cp.alloc(cp.size() + 1));
    SPK_TRY(d_out.alloc((size_t)n + 1));
    SPK_TRY(d_huge.alloc((size_t)n + 1));
    SPK_TRY(d_nhuge.alloc(1));
    SPK_HIP(hipMemsetAsync(d_nhuge.p, 0, sizeof(unsigned int), ctx->stream));  // hipMalloc does not zero
    SPK_HIP(hipMemcpyAsync(d_u.p, u.data(), u.size() * 2, hipMemcpyHostToDevice, ctx->stream));
    SPK_HIP(hipMemcpyAsync(d_off.p, off.data(), off.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    if (!cp.empty()) SPK_HIP(hipMemcpyAsync(d_cp.p, cp.data(), cp.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    if (!n) return SPK_OK;
    UdfArgs U{n, d_u.p, d_off.p, d_cp.p, op, d_out.p, d_huge.p, d_nhuge.p};
    const unsigned grid = (unsigned)((n + U_THREADS - 1) / U_THREADS);
    if (op >= 2) k_udf_set<<<grid, U_THREADS, 0, ctx->stream>>>(U);
    else k_udf<<<grid, U_THREADS, 0, ctx->stream>>>(U);
    SPK_HIP(hipGetLastError());
    unsigned int n_huge = 0;
    SPK_HIP(hipMemcpyAsync(&n_huge, d_nhuge.p, sizeof(n_huge), hipMemcpyDeviceToHost, ctx->stream));
    SPK_HIP(hipStreamSynchronize(ctx->stream));
    DevBuf<uint8_t> scratch;
    if (n_huge) {
        int64_t units = 1;
        for (size_t i = 0; i + 1 < off.size(); ++i) units = std::max<int64_t>(units, off[i + 1] - off[i]);
        Scratch S;
        SPK_TRY(huge_scratch(units, n_huge, scratch, S));
        if (op >= 2) k_udf_set_huge<<<(unsigned)(S.n_slots / 64), 64, 0, ctx->stream>>>(U, (int64_t)n_huge, S);
        else k_udf_huge<<<(unsigned)(S.n_slots / 64), 64, 0, ctx->stream>>>(U, (int64_t)n_huge, S);
        SPK_HIP(hipGetLastError());
    }
    SPK_HIP(hipMemcpyAsync(out, d_out.p, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
    SPK_HIP(hipStreamSynchronize(ctx->stream));
    return SPK_OK;
}

extern "C" int spk_jaro_winkler_sim(spk_ctx *ctx, int64_t n, const int64_t *l_off, const uint8_t *l_utf8,
                                    const int64_t *r_off, const uint8_t *r_utf8, double *out) {
    return run_udf(ctx, 0, n, l_off, l_utf8, r_off, r_utf8, out);
}

extern "C" int spk_levenshtein(spk_ctx *ctx, int64_t n, const int64_t *l_off, const uint8_t *l_utf8,
                               const int64_t *r_off, const uint8_t *r_utf8, double *out) {
    return run_udf(ctx, 1, n, l_off, l_utf8, r_off, r_utf8, out);
}

extern "C" int spk_jaccard_sim(spk_ctx *ctx, int64_t n, const int64_t *l_off, const uint8_t *l_utf8,
                               const int64_t *r_off, const uint8_t *r_utf8, double *out) {
    return run_udf(ctx, 2, n, l_off, l_utf8, r_off, r_utf8, out);
}

extern "C" int spk_cosine_distance(spk_ctx *ctx, int64_t n, const int64_t *l_off, const uint8_t *l_utf8,
                                   const int64_t *r_off, const uint8_t *r_utf8, double *out) {
    return run_udf(ctx, 3, n, l_off, l_utf8, r_off, r_utf8, out);
}
