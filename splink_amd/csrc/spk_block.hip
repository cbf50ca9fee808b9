// Candidate-pair generation (replaces blocking.py:95-318, Spark's per-rule equi-join + UNION ALL).
//
// Per rule: rows with a non-NULL key are radix-sorted by (key, rank); runs of equal keys are
// blocks.  Every block contributes a contiguous range of candidate ordinals (n(n-1)/2 for a
// symmetric self-join, nL*nR for a bipartite join), so the whole job is one int64 ordinal space
// that is cut into equal chunks regardless of block skew, and sharded evenly across GPUs.
// Each ordinal decodes to one (l, r) row pair; the earlier-rule exclusion and the link-type
// predicate are applied per pair.  Two passes (count, emit) keep the output in ordinal order,
// so pair order is deterministic and independent of the grid.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "spk_internal.h"
#include "spk_prim.h"

namespace spk {

static constexpr int EN_THREADS = 256;
static constexpr int EN_PER_THREAD = 8;
static constexpr int64_t EN_CHUNK = (int64_t)EN_THREADS * EN_PER_THREAD;
static constexpr int MAX_RULES = 32;

struct RuleKeys {
    const int64_t *keyL[MAX_RULES];  // key of rule j at each l-view position (position-ordered copy)
    const int64_t *keyR[MAX_RULES];  // key of rule j at each r-view position
};

// dst[i] = src[rows[i]]: a table array in a rule's view order, so k_enum reads it by view position
// (contiguous within a block) instead of gathering it by row for every candidate pair.
__global__ void k_by_position(int64_t n, const int32_t *__restrict__ rows, const int64_t *__restrict__ src,
                              int64_t *__restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[rows[i]];
}

// Grid-stride, valid keys counted per workgroup (ballots, then LDS): one atomic per workgroup -- an atomic
// per wave on the one counter serialised at L2 (187 us per million rows at cfg2).
__global__ void k_make_sort_keys(int64_t n, const int64_t *__restrict__ key, const int64_t *__restrict__ rank,
                                 uint64_t *__restrict__ out_keys, int32_t *__restrict__ out_rows,
                                 unsigned long long *__restrict__ n_valid) {
    __shared__ unsigned long long s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    unsigned long long cnt = 0;  // wave-uniform
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x; i0 < n; i0 += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = i0 + threadIdx.x;
        bool v = false;
        if (i < n) {
            const int64_t k = key[i];
            const uint64_t r = rank ? (uint64_t)rank[i] : 0ull;
            out_keys[i] = k < 0 ? ~0ull : (((uint64_t)k << 32) | r);
            out_rows[i] = (int32_t)i;
            v = k >= 0;
        }
        cnt += (unsigned long long)__popcll(__ballot(v));
    }
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&s_cnt, cnt);
    __syncthreads();
    if (threadIdx.x == 0 && s_cnt) atomicAdd(n_valid, s_cnt);
}

__global__ void k_heads(int64_t n, const uint64_t *__restrict__ keys, int64_t *__restrict__ flag) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    flag[i] = (i == 0 || (keys[i] >> 32) != (keys[i - 1] >> 32)) ? 1 : 0;
}

__global__ void k_starts(int64_t n, const int64_t *__restrict__ flag, const int64_t *__restrict__ pos,
                         int64_t *__restrict__ bstart) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (flag[i]) bstart[pos[i]] = i;
}

__device__ inline int64_t lower_bound_hi(const uint64_t *keys, int64_t n, uint64_t k) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        int64_t mid = (lo + hi) >> 1;
        if ((keys[mid] >> 32) < k) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// candidate count per block; bipartite blocks locate their r-side range by binary search.
__global__ void k_cand(int64_t B, const int64_t *__restrict__ bstart, int tri, const uint64_t *__restrict__ keysL,
                       const uint64_t *__restrict__ keysR, int64_t nR, int64_t *__restrict__ bstartR,
                       int64_t *__restrict__ bnR, int64_t *__restrict__ cand) {
    int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int64_t n = bstart[b + 1] - bstart[b];
    if (tri) {
        cand[b] = n * (n - 1) / 2;
        return;
    }
    uint64_t k = keysL[bstart[b]] >> 32;
    int64_t lo = lower_bound_hi(keysR, nR, k);
    int64_t hi = lower_bound_hi(keysR, nR, k + 1);
    bstartR[b] = lo;
    bnR[b] = hi - lo;
    cand[b] = n * (hi - lo);
}

struct EnumArgs {
    int64_t q0, q1;             // rule-local ordinal range of this shard
    int64_t B;
    const int64_t *cand_off;    // [B] exclusive prefix of candidates
    const int64_t *bstart;      // [B+1] l-view block starts
    const int64_t *bstartR;     // [B] r-view starts (bipartite)
    const int64_t *bnR;         // [B] r-view sizes (bipartite)
    const int32_t *rowsL, *rowsR;
    const int64_t *rankL, *rankR;  // rank at each l- / r-view position (position-ordered copies)
    int tri;
    int rank_filter;            // 1: keep rank(l) < rank(r) (dedupe / link_and_dedupe)
    int64_t null_div;           // > 0: rank = src * null_div + r, r == null_div - 1 for a NULL unique id
    int rule;                   // earlier rules that exclude their pairs on the key alone: keys.key*[0 .. rule)
    RuleKeys keys;
    int64_t *chunk_count;       // count pass output
    const int64_t *chunk_off;   // emit pass input
    int32_t *out_l, *out_r;
    int32_t *out_vl, *out_vr;   // emit pass: view positions (rules with a view), or null
};

__device__ inline int64_t tri_s(int64_t a, int64_t n) { return a * (2 * n - a - 1) / 2; }

template <bool EMIT>
__global__ __launch_bounds__(EN_THREADS) void k_enum(EnumArgs A) {
    __shared__ int64_t s_scan[EN_THREADS];
    const int64_t chunk = blockIdx.x;
    const int64_t base = A.q0 + chunk * EN_CHUNK + (int64_t)threadIdx.x * EN_PER_THREAD;
    int32_t xs[EN_PER_THREAD], ys[EN_PER_THREAD], vx[EN_PER_THREAD], vy[EN_PER_THREAD];
    unsigned keep = 0;
    if (base < A.q1) {
        // block containing `base`: last b with cand_off[b] <= base
        int64_t lo = 0, hi = A.B;
        while (hi - lo > 1) {
            int64_t mid = (lo + hi) >> 1;
            if (A.cand_off[mid] <= base) lo = mid;
            else hi = mid;
        }
        int64_t b = lo;
        int64_t w = base - A.cand_off[b];
        int64_t n = A.bstart[b + 1] - A.bstart[b];
        int64_t nr = A.tri ? n : A.bnR[b];
        int64_t cand_b = A.tri ? n * (n - 1) / 2 : n * nr;
        while (w >= cand_b) {  // skip empty blocks
            w -= cand_b;
            ++b;
            n = A.bstart[b + 1] - A.bstart[b];
            nr = A.tri ? n : A.bnR[b];
            cand_b = A.tri ? n * (n - 1) / 2 : n * nr;
        }
        int64_t a, c;
        if (A.tri) {
            double tn = 2.0 * (double)n - 1.0;
            double disc = tn * tn - 8.0 * (double)w;
            a = (int64_t)((tn - sqrt(disc > 0 ? disc : 0.0)) * 0.5);
            if (a < 0) a = 0;
            while (a > 0 && tri_s(a, n) > w) --a;
            while (a + 1 < n && tri_s(a + 1, n) <= w) ++a;
            c = a + 1 + (w - tri_s(a, n));
        } else {
            a = w / nr;
            c = w - a * nr;
        }
        for (int i = 0; i < EN_PER_THREAD; ++i) {
            int64_t q = base + i;
            if (q >= A.q1) break;
            if (i > 0) {  // advance to the next ordinal
                ++c;
                if (c >= nr) {
                    ++a;
                    c = A.tri ? a + 1 : 0;
                    if (a >= (A.tri ? n - 1 : n)) {
                        do {
                            ++b;
                            n = A.bstart[b + 1] - A.bstart[b];
                            nr = A.tri ? n : A.bnR[b];
                        } while ((A.tri ? n * (n - 1) / 2 : n * nr) == 0);
                        a = 0;
                        c = A.tri ? 1 : 0;
                    }
                }
            }
            const int64_t pa = A.bstart[b] + a, pc = A.tri ? A.bstart[b] + c : A.bstartR[b] + c;
            int32_t x = A.rowsL[pa];
            int32_t y = A.tri ? A.rowsL[pc] : A.rowsR[pc];
            vx[i] = (int32_t)pa;
            vy[i] = (int32_t)pc;
            bool ok = true;
            if (A.rank_filter) {
                int64_t rx = A.rankL[pa], ry = A.rankR[pc];
                if (A.tri) {
                    ok = rx != ry;  // sorted by rank inside the block: rx <= ry
                } else {
                    ok = rx < ry;
                }
                // `l.uid < r.uid` is NULL (the pair is dropped) when either unique id is NULL; pairs
                // across the two sources of link_and_dedupe are kept by `l.src < r.src` alone
                if (ok && A.null_div > 0 && rx / A.null_div == ry / A.null_div &&
                    (rx % A.null_div == A.null_div - 1 || ry % A.null_div == A.null_div - 1))
                    ok = false;
            }
            for (int j = 0; ok && j < A.rule; ++j) {
                int64_t kl = A.keys.keyL[j][pa];
                if (kl >= 0 && kl == A.keys.keyR[j][pc]) ok = false;
            }
            xs[i] = x;
            ys[i] = y;
            if (ok) keep |= 1u << i;
        }
    }
    int cnt = __popc(keep);
    // block-wide exclusive scan of the per-thread counts (Hillis-Steele in LDS)
    s_scan[threadIdx.x] = cnt;
    __syncthreads();
    for (int off = 1; off < EN_THREADS; off <<= 1) {
        int64_t v = threadIdx.x >= off ? s_scan[threadIdx.x - off] : 0;
        __syncthreads();
        s_scan[threadIdx.x] += v;
        __syncthreads();
    }
    int64_t incl = s_scan[threadIdx.x];
    if (!EMIT) {
        if (threadIdx.x == EN_THREADS - 1) A.chunk_count[chunk] = incl;
        return;
    }
    // the block's kept pairs are compacted in LDS, then written out with consecutive lanes on
    // consecutive positions (a thread's own run of EN_PER_THREAD would give strided lane writes)
    __shared__ int32_t s_out[4][EN_CHUNK];
    const bool views = A.out_vl != nullptr;
    int loc = (int)(incl - cnt);
    for (int i = 0; i < EN_PER_THREAD; ++i) {
        if (keep & (1u << i)) {
            s_out[0][loc] = xs[i];
            s_out[1][loc] = ys[i];
            if (views) {
                s_out[2][loc] = vx[i];
                s_out[3][loc] = vy[i];
            }
            ++loc;
        }
    }
    __syncthreads();
    const int total = (int)s_scan[EN_THREADS - 1];
    const int64_t out0 = A.chunk_off[chunk];
    for (int k = threadIdx.x; k < total; k += EN_THREADS) {
        A.out_l[out0 + k] = s_out[0][k];
        A.out_r[out0 + k] = s_out[1][k];
        if (views) {
            A.out_vl[out0 + k] = s_out[2][k];
            A.out_vr[out0 + k] = s_out[3][k];
        }
    }
}

struct SortedView {
    DevBuf<uint64_t> keys;
    DevBuf<int32_t> rows;
    int64_t n_valid = 0;
};

static int sort_view(spk_ctx *ctx, int64_t n, const int64_t *d_key, const int64_t *d_rank, SortedView &v,
                     DevBuf<uint8_t> &tmp) {
    DevBuf<uint64_t> k_in;
    DevBuf<int32_t> r_in;
    DevBuf<unsigned long long> cnt;
    SPK_TRY(k_in.alloc((size_t)n + 1));
    SPK_TRY(r_in.alloc((size_t)n + 1));
    SPK_TRY(v.keys.alloc((size_t)n + 1));
    SPK_TRY(v.rows.alloc((size_t)n + 1));
    SPK_TRY(cnt.alloc(1));
    SPK_HIP(hipMemsetAsync(cnt.p, 0, sizeof(unsigned long long), ctx->stream));
    if (n == 0) {
        v.n_valid = 0;
        return SPK_OK;
    }
    k_make_sort_keys<<<(unsigned)std::min<int64_t>((n + 255) / 256, 4 * (int64_t)ctx->n_cu), 256, 0, ctx->stream>>>(
        n, d_key, d_rank, k_in.p, r_in.p, cnt.p);
    SPK_HIP(hipGetLastError());
    SPK_TRY(sort_pairs_u64(ctx->stream, tmp, k_in.p, v.keys.p, r_in.p, v.rows.p, n));
    unsigned long long h = 0;
    SPK_HIP(hipMemcpyAsync(&h, cnt.p, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    SPK_HIP(hipStreamSynchronize(ctx->stream));
    v.n_valid = (int64_t)h;
    return SPK_OK;
}

struct RulePlan {
    SortedView L, R;
    DevBuf<int64_t> bstart, bstartR, bnR;
    CountScan cand;  // candidates per block; cand.total: the rule's candidate ordinals
    // by view position: rank (l, r), then the keys of the earlier rules (l then r per rule)
    DevBuf<int64_t> bypos;
    const int64_t *rankL = nullptr, *rankR = nullptr;
    const int64_t *keyL[MAX_RULES] = {}, *keyR[MAX_RULES] = {};
    int n_excl = 0;  // earlier rules whose keys are in keyL / keyR
    int64_t B = 0;
    int tri = 1;
};

static int plan_rule(spk_ctx *ctx, int rule, bool symmetric, RulePlan &P, DevBuf<uint8_t> &tmp) {
    Table &tl = ctx->table[0];
    Table &tr = ctx->side_table(1);
    bool link_only = ctx->link_type == SPK_LINK_ONLY;
    P.tri = (symmetric && !link_only) ? 1 : 0;
    const int64_t *rankL = tl.rank.p;
    SPK_TRY(sort_view(ctx, tl.n, tl.key[0][rule]->p, link_only ? nullptr : rankL, P.L, tmp));
    if (!P.tri) SPK_TRY(sort_view(ctx, tr.n, tr.key[1][rule]->p, nullptr, P.R, tmp));
    int64_t n = P.L.n_valid;
    if (n == 0) return SPK_OK;
    CountScan heads;
    SPK_TRY(heads.alloc(ctx, n));
    unsigned g = (unsigned)((n + 255) / 256);
    k_heads<<<g, 256, 0, ctx->stream>>>(n, P.L.keys.p, heads.count.p);
    SPK_TRY(scan_total(ctx, heads, tmp));
    const int64_t B = P.B = heads.total;
    SPK_TRY(P.bstart.alloc((size_t)B + 1));
    SPK_TRY(P.bstartR.alloc((size_t)B + 1));
    SPK_TRY(P.bnR.alloc((size_t)B + 1));
    SPK_TRY(P.cand.alloc(ctx, B));
    k_starts<<<g, 256, 0, ctx->stream>>>(n, heads.count.p, heads.off.p, P.bstart.p);
    SPK_HIP(hipMemcpyAsync(P.bstart.p + B, &n, 8, hipMemcpyHostToDevice, ctx->stream));
    k_cand<<<(unsigned)((B + 255) / 256), 256, 0, ctx->stream>>>(B, P.bstart.p, P.tri, P.L.keys.p,
                                                                 P.tri ? nullptr : P.R.keys.p, P.R.n_valid,
                                                                 P.bstartR.p, P.bnR.p, P.cand.count.p);
    SPK_HIP(hipGetLastError());
    return scan_total(ctx, P.cand, tmp);
}

// Position-ordered copies of what k_enum reads per candidate pair: ranks (dedupe / link_and_dedupe) and
// the keys of the earlier rules in `excl` (earlier-rule exclusion: every earlier rule, except those with a
// residual predicate -- a key match with such a rule does not exclude the pair, spk_block_residual).  Built
// just before a pass over the rule and released after it (release_by_position), so at most one rule's copies
// exist at a time; a symmetric self-join (tri) reads the l-side rank copy for both sides.
static int build_by_position(spk_ctx *ctx, const std::vector<int> &excl, RulePlan &P) {
    const int rule = (int)excl.size();
    Table &tl = ctx->table[0];
    Table &tr = ctx->side_table(1);
    const bool ranks = ctx->link_type != SPK_LINK_ONLY;
    const int64_t nL = P.L.n_valid, nR = P.tri ? nL : P.R.n_valid;
    const int32_t *rowsR = P.tri ? P.L.rows.p : P.R.rows.p;
    const int64_t n_rank = ranks ? (P.tri ? nL : nL + nR) : 0;
    SPK_TRY(P.bypos.alloc((size_t)(n_rank + (int64_t)rule * (nL + nR)) + 1));
    int64_t *at = P.bypos.p;
    auto by_pos = [&](int64_t m, const int32_t *rows, const int64_t *src) -> const int64_t * {
        int64_t *dst = at;
        at += m;
        if (m > 0) k_by_position<<<(unsigned)((m + 255) / 256), 256, 0, ctx->stream>>>(m, rows, src, dst);
        return dst;
    };
    if (ranks) {
        P.rankL = by_pos(nL, P.L.rows.p, tl.rank.p);
        P.rankR = P.tri ? P.rankL : by_pos(nR, rowsR, tr.rank.p);
    }
    for (int j = 0; j < rule; ++j) {
        P.keyL[j] = by_pos(nL, P.L.rows.p, tl.key[0][excl[j]]->p);
        P.keyR[j] = by_pos(nR, rowsR, tr.key[1][excl[j]]->p);
    }
    P.n_excl = rule;
    SPK_HIP(hipGetLastError());
    return SPK_OK;
}

static void release_by_position(RulePlan &P) {
    P.bypos.release();
    P.rankL = P.rankR = nullptr;
    for (int j = 0; j < MAX_RULES; ++j) P.keyL[j] = P.keyR[j] = nullptr;
    P.n_excl = 0;
}

// k_enum's arguments for the ordinals [q0, q1) of a rule whose by-position copies are built.  The count pass
// adds chunk_count, the emit pass chunk_off and the outputs: everything both passes must agree on is set here.
static EnumArgs enum_args(spk_ctx *ctx, const RulePlan &P, int64_t q0, int64_t q1) {
    EnumArgs A{};
    A.q0 = q0;
    A.q1 = q1;
    A.B = P.B;
    A.cand_off = P.cand.off.p;
    A.bstart = P.bstart.p;
    A.bstartR = P.bstartR.p;
    A.bnR = P.bnR.p;
    A.rowsL = P.L.rows.p;
    A.rowsR = P.tri ? P.L.rows.p : P.R.rows.p;
    A.rankL = P.rankL;
    A.rankR = P.rankR;
    A.tri = P.tri;
    A.rank_filter = ctx->link_type == SPK_LINK_ONLY ? 0 : 1;
    A.null_div = ctx->table[0].null_div;
    A.rule = P.n_excl;
    for (int j = 0; j < P.n_excl; ++j) {
        A.keys.keyL[j] = P.keyL[j];
        A.keys.keyR[j] = P.keyR[j];
    }
    return A;
}

// ---- residual predicates: stable compaction of one rule's pair range by the hidden programs' codes -------
// A workgroup takes RF_CHUNK consecutive ordinals as RF_SLABS slabs of RF_THREADS, so that a wave's lanes hold
// consecutive pairs: a ballot gives the wave's kept pairs in ordinal order, the four waves' counts go through
// LDS, and every kept pair is written at chunk offset + kept pairs before it -- consecutive kept lanes on
// consecutive positions, the order of the ordinals (no atomics).  Count pass, exclusive scan of the chunk
// counts, emit pass, as k_enum.
static constexpr int RF_THREADS = 256;
static constexpr int RF_SLABS = 8;
static constexpr int64_t RF_CHUNK = (int64_t)RF_THREADS * RF_SLABS;
static constexpr int RF_WAVES = RF_THREADS / 64;

struct ResidualFilterArgs {
    int64_t lo, hi;             // the rule's ordinals in the enumerated pair set
    const uint16_t *codes;      // the hidden programs' packed codes, one per enumerated pair
    const uint8_t *keep;        // [n_patterns] 1: a pair of this rule with that code survives
    int64_t n_patterns;
    const int32_t *in_l, *in_r;    // enumerated pairs (indexed by ordinal)
    const int32_t *in_vl, *in_vr;  // their view positions from ordinal v_lo on, or null (rule without a view)
    int64_t v_lo;
    int64_t *chunk_count;       // count pass output
    const int64_t *chunk_off;   // emit pass input
    int32_t *out_l, *out_r;     // emit pass: the rule's survivors from its new first ordinal on
    int32_t *out_vl, *out_vr;
};

template <bool EMIT>
__global__ __launch_bounds__(RF_THREADS) void k_residual_filter(ResidualFilterArgs A) {
    __shared__ int s_wave[RF_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t base = A.lo + (int64_t)blockIdx.x * RF_CHUNK;
    int64_t run = EMIT ? A.chunk_off[blockIdx.x] : 0;  // kept pairs of the rule before this slab
    int wave_total = 0;                                // count pass: this wave's kept pairs (wave-uniform)
    for (int s = 0; s < RF_SLABS; ++s) {
        const int64_t p = base + (int64_t)s * RF_THREADS + threadIdx.x;
        bool k = false;
        if (p < A.hi) {
            const int64_t c = A.codes[p];
            k = c < A.n_patterns && A.keep[c] != 0;
        }
        const unsigned long long m = __ballot(k);
        const int n = __popcll(m);
        if (!EMIT) {
            wave_total += n;
            continue;
        }
        if (lane == 0) s_wave[wave] = n;
        __syncthreads();
        int before = 0, all = 0;
        for (int w = 0; w < RF_WAVES; ++w) {
            const int c = s_wave[w];
            before += w < wave ? c : 0;
            all += c;
        }
        if (k) {
            const int64_t q = run + before + __popcll(m & ((1ull << lane) - 1ull));
            A.out_l[q] = A.in_l[p];
            A.out_r[q] = A.in_r[p];
            if (A.in_vl) {
                A.out_vl[q] = A.in_vl[p - A.v_lo];
                A.out_vr[q] = A.in_vr[p - A.v_lo];
            }
        }
        run += all;
        __syncthreads();  // s_wave is rewritten by the next slab
    }
    if (!EMIT) {
        if (lane == 0) s_wave[wave] = wave_total;
        __syncthreads();
        if (threadIdx.x == 0) {
            int64_t t = 0;
            for (int w = 0; w < RF_WAVES; ++w) t += s_wave[w];
            A.chunk_count[blockIdx.x] = t;
        }
    }
}

// ---- rule profile (spk_block_profile): block statistics and the largest blocks of a planned rule --------------
static constexpr int PS_THREADS = 256;
static constexpr int PS_WAVES = PS_THREADS / 64;
static constexpr int64_t PROFILE_SLAB = (int64_t)1 << 31;  // ordinals per count-pass launch (a multiple of EN_CHUNK)

struct ProfileStats {
    unsigned long long hist[SPK_PROFILE_BINS][2];      // by bit length of the candidate count: blocks, candidates
    unsigned long long rows_bins[SPK_PROFILE_BINS];    // by bit length of the l-side row count: blocks
    unsigned long long largest;                        // candidates of the largest block
};

__device__ inline int bit_length(int64_t v) { return v > 0 ? 64 - __clzll((long long)v) : 0; }

// One pass over the per-block candidate counts.  A workgroup bins into LDS counters and adds each non-empty one to
// the global counters once; the largest count goes through a wave reduction and one atomicMax per workgroup.  Every
// counter is an integer, so the result does not depend on the launch shape.
__global__ __launch_bounds__(PS_THREADS) void k_block_stats(int64_t B, const int64_t *__restrict__ cand,
                                                            const int64_t *__restrict__ bstart,
                                                            ProfileStats *__restrict__ out) {
    __shared__ unsigned long long s_bins[SPK_PROFILE_BINS][3];
    __shared__ long long s_max[PS_WAVES];
    if (threadIdx.x < SPK_PROFILE_BINS) s_bins[threadIdx.x][0] = s_bins[threadIdx.x][1] = s_bins[threadIdx.x][2] = 0;
    __syncthreads();
    long long mx = 0;
    for (int64_t b = (int64_t)blockIdx.x * PS_THREADS + threadIdx.x; b < B; b += (int64_t)gridDim.x * PS_THREADS) {
        const int64_t c = cand[b];
        const int i = bit_length(c);
        atomicAdd(&s_bins[i][0], 1ull);
        if (c > 0) atomicAdd(&s_bins[i][1], (unsigned long long)c);
        atomicAdd(&s_bins[bit_length(bstart[b + 1] - bstart[b])][2], 1ull);
        mx = c > mx ? c : mx;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const long long o = __shfl_xor(mx, off, 64);
        mx = o > mx ? o : mx;
    }
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long m = 0;
        for (int w = 0; w < PS_WAVES; ++w) m = s_max[w] > m ? s_max[w] : m;
        if (m > 0) atomicMax(&out->largest, (unsigned long long)m);
    }
    if (threadIdx.x < SPK_PROFILE_BINS) {
        const int i = threadIdx.x;
        if (s_bins[i][0]) atomicAdd(&out->hist[i][0], s_bins[i][0]);
        if (s_bins[i][1]) atomicAdd(&out->hist[i][1], s_bins[i][1]);
        if (s_bins[i][2]) atomicAdd(&out->rows_bins[i], s_bins[i][2]);
    }
}

// What the largest blocks are ordered by: the candidate count, or the l-side rows.
__device__ inline int64_t block_metric(int by_rows, const int64_t *cand, const int64_t *bstart, int64_t b) {
    return by_rows ? bstart[b + 1] - bstart[b] : cand[b];
}

// Blocks whose metric lies in the bins >= min_bin, compacted in block order (count, scan, emit): the sort key is the
// complement of the metric, so an ascending stable sort gives descending metric with ties in ascending block index.
__global__ void k_top_flag(int64_t B, const int64_t *__restrict__ cand, const int64_t *__restrict__ bstart, int by_rows,
                           int min_bin, int64_t *__restrict__ flag) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) flag[b] = bit_length(block_metric(by_rows, cand, bstart, b)) >= min_bin ? 1 : 0;
}

__global__ void k_top_emit(int64_t B, const int64_t *__restrict__ cand, const int64_t *__restrict__ bstart, int by_rows,
                           const int64_t *__restrict__ flag, const int64_t *__restrict__ off,
                           uint64_t *__restrict__ keys, int32_t *__restrict__ index) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B || !flag[b]) return;
    keys[off[b]] = ~(uint64_t)block_metric(by_rows, cand, bstart, b);
    index[off[b]] = (int32_t)b;
}

__global__ void k_top_entries(int m, const int32_t *__restrict__ index, const int64_t *__restrict__ cand,
                              const int64_t *__restrict__ bstart, const int64_t *__restrict__ bnR, int tri,
                              const int32_t *__restrict__ rowsL, spk_block_entry *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const int64_t b = index[i];
    spk_block_entry e;
    e.rows_l = bstart[b + 1] - bstart[b];
    e.rows_r = tri ? e.rows_l : bnR[b];
    e.candidates = cand[b];
    e.row_l = rowsL[bstart[b]];
    e.pad = 0;
    out[i] = e;
}

}  // namespace spk

using namespace spk;

extern "C" int spk_ctx_set_link_type(spk_ctx *ctx, int link_type) {
    SPK_REQUIRE(ctx && link_type >= 0 && link_type <= 2, SPK_E_INVALID, "bad link_type");
    ctx->link_type = link_type;
    return SPK_OK;
}

// spk_block / the enumeration of spk_block_residual.  rule_program: null, or per rule the index of its residual
// predicate's program (-1: the rule is only its key equalities); an earlier rule with a program does not exclude
// on its key, so k_enum gets the keys of the other earlier rules only (with no program anywhere: all of them).
static int block_rules(spk_ctx *ctx, int link_type, int n_rules, const int32_t *rule_symmetric,
                       const int32_t *rule_program, int shard, int n_shards, int64_t *out_n_pairs,
                       int64_t *out_n_candidates_total) {
    SPK_REQUIRE(ctx && n_rules >= 1 && n_rules <= MAX_RULES && rule_symmetric, SPK_E_INVALID,
                "spk_block: need 1..32 rules");
    SPK_REQUIRE(link_type >= 0 && link_type <= 2, SPK_E_INVALID, "spk_block: bad link_type");
    SPK_REQUIRE(n_shards >= 1 && shard >= 0 && shard < n_shards, SPK_E_INVALID, "spk_block: bad shard");
    SPK_HIP(hipSetDevice(ctx->device));
    ctx->link_type = link_type;
    Table &tl = ctx->table[0];
    Table &tr = ctx->side_table(1);
    SPK_REQUIRE(tl.n >= 0 && tr.n >= 0, SPK_E_STATE, "spk_block: tables not loaded");
    bool link_only = link_type == SPK_LINK_ONLY;
    SPK_REQUIRE(link_only || tl.rank.p || tl.n == 0, SPK_E_STATE, "spk_block: rank not set");
    for (int r = 0; r < n_rules; ++r) {
        SPK_REQUIRE((int)tl.key[0].size() > r && tl.key[0][r]->p && (int)tr.key[1].size() > r && tr.key[1][r]->p,
                    SPK_E_STATE, "spk_block: keys not set for every rule");
    }
    SPK_TRY(ctx->begin(K_BLOCK));
    DevBuf<uint8_t> tmp;
    std::vector<RulePlan> plans(n_rules);
    int64_t total = 0;
    for (int r = 0; r < n_rules; ++r) {
        SPK_TRY(plan_rule(ctx, r, rule_symmetric[r] != 0, plans[r], tmp));
        total += plans[r].cand.total;
    }
    int64_t g_lo = (int64_t)((__int128)total * shard / n_shards);
    int64_t g_hi = (int64_t)((__int128)total * (shard + 1) / n_shards);

    std::vector<std::vector<int>> excl(n_rules);
    for (int r = 0; r < n_rules; ++r)
        for (int j = 0; j < r; ++j)
            if (!rule_program || rule_program[j] < 0) excl[r].push_back(j);
    // count pass
    struct Pass {
        int64_t lo = 0, hi = 0;  // this shard's ordinals of the rule (rule-local)
        CountScan chunks;        // pairs kept per EN_CHUNK ordinals; n = 0: the shard has none of the rule
    };
    std::vector<Pass> pass(n_rules);
    std::vector<int64_t> rule_base(n_rules);
    int64_t acc = 0, n_out = 0;
    for (int r = 0; r < n_rules; ++r) {
        RulePlan &P = plans[r];
        Pass &Q = pass[r];
        Q.lo = std::max<int64_t>(g_lo - acc, 0);
        Q.hi = std::min<int64_t>(g_hi - acc, P.cand.total);
        acc += P.cand.total;
        rule_base[r] = n_out;
        if (Q.hi <= Q.lo) continue;
        SPK_TRY(build_by_position(ctx, excl[r], P));
        SPK_TRY(Q.chunks.alloc(ctx, (Q.hi - Q.lo + EN_CHUNK - 1) / EN_CHUNK));
        EnumArgs A = enum_args(ctx, P, Q.lo, Q.hi);
        A.chunk_count = Q.chunks.count.p;
        k_enum<false><<<(unsigned)Q.chunks.n, EN_THREADS, 0, ctx->stream>>>(A);
        SPK_HIP(hipGetLastError());
        SPK_TRY(scan_total(ctx, Q.chunks, tmp));  // synchronises: the pass is done, its copies can be freed
        release_by_position(P);
        n_out += Q.chunks.total;
    }
    SPK_REQUIRE(n_out < (int64_t)1 << 40, SPK_E_LIMIT, "spk_block: pair count too large");
    SPK_TRY(ctx->pl.alloc((size_t)n_out + 1));
    SPK_TRY(ctx->pr.alloc((size_t)n_out + 1));
    // rules 1 .. MAX_VIEWS-1 keep their row order (view) and emit their pairs' view positions
    const int n_views = std::min(n_rules, MAX_VIEWS) - 1;
    const int64_t pv_base = view_pair_base(rule_base, n_out);
    ctx->n_views = 0;  // no view until this call's are in place (set_rule_ranges)
    if (n_views > 0 && n_out > pv_base) {
        SPK_TRY(ctx->pvl.alloc((size_t)(n_out - pv_base) + 1));
        SPK_TRY(ctx->pvr.alloc((size_t)(n_out - pv_base) + 1));
    }
    for (int r = 0; r < n_rules; ++r) {
        Pass &Q = pass[r];
        if (!Q.chunks.n) continue;
        RulePlan &P = plans[r];
        SPK_TRY(build_by_position(ctx, excl[r], P));
        EnumArgs A = enum_args(ctx, P, Q.lo, Q.hi);
        A.chunk_off = Q.chunks.off.p;
        A.out_l = ctx->pl.p + rule_base[r];
        A.out_r = ctx->pr.p + rule_base[r];
        const bool view = r >= 1 && r <= n_views;
        A.out_vl = view ? ctx->pvl.p + (rule_base[r] - pv_base) : nullptr;
        A.out_vr = view ? ctx->pvr.p + (rule_base[r] - pv_base) : nullptr;
        k_enum<true><<<(unsigned)Q.chunks.n, EN_THREADS, 0, ctx->stream>>>(A);
        SPK_HIP(hipGetLastError());
        SPK_HIP(hipStreamSynchronize(ctx->stream));
        release_by_position(P);
    }
    SPK_TRY(ctx->end(K_BLOCK));
    SPK_HIP(hipStreamSynchronize(ctx->stream));
    for (int r = 1; r <= n_views; ++r) {
        RuleView &v = ctx->views[r];
        RulePlan &P = plans[r];
        v.rowsL = std::move(P.L.rows);
        v.nL = P.L.n_valid;
        v.tri = P.tri != 0;
        if (!v.tri) v.rowsR = std::move(P.R.rows);
        else v.rowsR.release();
        v.nR = v.tri ? v.nL : P.R.n_valid;
    }
    ctx->pair_terms.assign(ctx->rule_terms, ctx->rule_terms + n_rules);
    ctx->pairs_replaced(n_out);
    ctx->set_rule_ranges(rule_base, n_out);
    if (out_n_pairs) *out_n_pairs = n_out;
    if (out_n_candidates_total) *out_n_candidates_total = total;
    return SPK_OK;
}

extern "C" int spk_block(spk_ctx *ctx, int link_type, int n_rules, const int32_t *rule_symmetric, int shard,
                         int n_shards, int64_t *out_n_pairs, int64_t *out_n_candidates_total) {
    return block_rules(ctx, link_type, n_rules, rule_symmetric, nullptr, shard, n_shards, out_n_pairs,
                       out_n_candidates_total);
}

namespace {
// Until spk_block_residual has replaced the enumerated candidates by the survivors, a failure leaves no pair set.
struct PairsCommit {
    spk_ctx *ctx;
    bool done = false;
    ~PairsCommit() {
        if (!done) ctx->pairs_dropped();
    }
};
}  // namespace

extern "C" int spk_block_residual(spk_ctx *ctx, int link_type, int n_rules, const int32_t *rule_symmetric,
                                  const int32_t *rule_program, int shard, int n_shards, int n_cols,
                                  const spk_column_program *cols, int n_when, const int32_t *when_first_instr,
                                  const int32_t *when_n_instr, const int32_t *when_level, int n_instr,
                                  const spk_instr *instr, int n_operands, const spk_operand *operands, int n_lits,
                                  const int64_t *lit_offsets, const uint8_t *lit_utf8, int64_t *out_n_pairs,
                                  int64_t *out_n_candidates_total) {
    SPK_REQUIRE(ctx && n_rules >= 1 && n_rules <= MAX_RULES && rule_symmetric && rule_program, SPK_E_INVALID,
                "spk_block_residual: need 1..32 rules");
    SPK_REQUIRE(n_cols >= 0 && n_cols <= SPK_MAX_RESIDUAL_RULES, SPK_E_LIMIT,
                "spk_block_residual: at most 8 rules may carry a residual predicate");
    bool any = false;
    std::vector<char> used((size_t)n_cols, 0);
    for (int r = 0; r < n_rules; ++r) {
        SPK_REQUIRE(rule_program[r] >= -1 && rule_program[r] < n_cols, SPK_E_INVALID,
                    "spk_block_residual: rule_program out of range");
        if (rule_program[r] < 0) continue;
        SPK_REQUIRE(!used[rule_program[r]], SPK_E_INVALID, "spk_block_residual: one program per rule");
        used[rule_program[r]] = 1;
        any = true;
    }
    SPK_REQUIRE(!any || cols, SPK_E_INVALID, "spk_block_residual: no programs");
    for (int k = 0; any && k < n_cols; ++k)
        SPK_REQUIRE(cols[k].n_levels == 2 && cols[k].else_level == 0, SPK_E_INVALID,
                    "spk_block_residual: a rule's predicate is a 2-level program (level 1: the rule is TRUE)");
    ctx->pairs_dropped();  // (the codes go with the first stage's pair set at the latest)
    PairsCommit commit{ctx};
    // ---- a. enumerate: the key candidates, excluded only by earlier rules without a predicate
    int64_t n_enum = 0, total = 0;
    SPK_TRY(block_rules(ctx, link_type, n_rules, rule_symmetric, rule_program, shard, n_shards, &n_enum, &total));
    ctx->res_enumerated = n_enum;
    ctx->res_filter_ms = -1.0;
    if (out_n_candidates_total) *out_n_candidates_total = total;
    if (!any || n_enum == 0) {  // nothing to evaluate: the pair set is spk_block's
        if (out_n_pairs) *out_n_pairs = n_enum;
        commit.done = true;
        return SPK_OK;
    }
    // ---- b. evaluate: the predicates over the enumerated candidates, as comparison columns of a pass of their own
    SPK_TRY(spk_gammas(ctx, n_cols, cols, n_when, when_first_instr, when_n_instr, when_level, n_instr, instr,
                       n_operands, operands, n_lits, lit_offsets, lit_utf8));
    SPK_TRY(settle_gammas(ctx, nullptr));
    SPK_REQUIRE(ctx->codes_valid && ctx->code_bytes == 2, SPK_E_STATE, "spk_block_residual: predicate codes");
    const int64_t n_pat = ctx->n_patterns;  // 3^n_cols
    // ---- c. filter.  keep[r][code]: rule r's own predicate is TRUE (digit 2 = level 1) and no earlier rule's is
    std::vector<uint8_t> keep((size_t)n_rules * (size_t)n_pat, 0);
    for (int r = 0; r < n_rules; ++r) {
        for (int64_t c = 0; c < n_pat; ++c) {
            auto is_true = [&](int k) { return (c / ctx->stride[k]) % 3 == 2; };
            bool ok = rule_program[r] < 0 || is_true(rule_program[r]);
            for (int j = 0; ok && j < r; ++j)
                if (rule_program[j] >= 0 && is_true(rule_program[j])) ok = false;
            keep[(size_t)r * (size_t)n_pat + (size_t)c] = ok ? 1 : 0;
        }
    }
    DevBuf<uint8_t> d_keep, tmp;
    SPK_TRY(d_keep.alloc(keep.size()));
    SPK_HIP(hipMemcpyAsync(d_keep.p, keep.data(), keep.size(), hipMemcpyHostToDevice, ctx->stream));
    // device time of the compaction alone: each rule's count kernel and scan, then the emit kernels; the host
    // round trips between them (the survivor counts, the allocations) lie outside the intervals
    StageTimer T{ctx};
    const int64_t old_pv_base = ctx->pv_base;
    const int n_views = ctx->n_views;
    // k_residual_filter's arguments for rule r's enumerated range: what both passes must agree on.  The count pass
    // adds chunk_count, the emit pass chunk_off, the outputs and the view positions.
    auto filter_args = [&](int r) {
        ResidualFilterArgs A{};
        A.lo = ctx->pair_rule_lo[r];
        A.hi = ctx->pair_rule_hi[r];
        A.codes = reinterpret_cast<const uint16_t *>(ctx->codes.p);
        A.keep = d_keep.p + (size_t)r * (size_t)n_pat;
        A.n_patterns = n_pat;
        A.in_l = ctx->pl.p;
        A.in_r = ctx->pr.p;
        return A;
    };
    std::vector<CountScan> chunks(n_rules);  // survivors per RF_CHUNK ordinals; n = 0: the rule enumerated nothing
    std::vector<int64_t> new_base(n_rules);
    int64_t n_out = 0;
    for (int r = 0; r < n_rules; ++r) {
        const int64_t lo = ctx->pair_rule_lo[r], hi = ctx->pair_rule_hi[r];
        new_base[r] = n_out;
        if (hi <= lo) continue;
        SPK_TRY(chunks[r].alloc(ctx, (hi - lo + RF_CHUNK - 1) / RF_CHUNK));
        ResidualFilterArgs A = filter_args(r);
        A.chunk_count = chunks[r].count.p;
        SPK_TRY(T.open());
        k_residual_filter<false><<<(unsigned)chunks[r].n, RF_THREADS, 0, ctx->stream>>>(A);
        SPK_HIP(hipGetLastError());
        SPK_TRY(scan_total(ctx, chunks[r], tmp, &T));
        n_out += chunks[r].total;
    }
    SPK_REQUIRE(n_out <= n_enum, SPK_E_STATE, "spk_block_residual: survivor count");
    // fresh buffers (both pair sets are held until the swap), rule 1's view positions with the same offsets
    DevBuf<int32_t> npl, npr, npvl, npvr;
    SPK_TRY(npl.alloc((size_t)n_out + 1));
    SPK_TRY(npr.alloc((size_t)n_out + 1));
    const int64_t pv_base = view_pair_base(new_base, n_out);
    if (n_views > 0 && n_out > pv_base) {
        SPK_TRY(npvl.alloc((size_t)(n_out - pv_base) + 1));
        SPK_TRY(npvr.alloc((size_t)(n_out - pv_base) + 1));
    }
    SPK_TRY(T.open());
    for (int r = 0; r < n_rules; ++r) {
        if (!chunks[r].n) continue;
        ResidualFilterArgs A = filter_args(r);
        A.chunk_off = chunks[r].off.p;
        A.out_l = npl.p + new_base[r];
        A.out_r = npr.p + new_base[r];
        const bool view = r >= 1 && r <= n_views && npvl.p && ctx->pvl.p;
        if (view) {
            A.in_vl = ctx->pvl.p;
            A.in_vr = ctx->pvr.p;
            A.v_lo = old_pv_base;
            A.out_vl = npvl.p + (new_base[r] - pv_base);
            A.out_vr = npvr.p + (new_base[r] - pv_base);
        }
        k_residual_filter<true><<<(unsigned)chunks[r].n, RF_THREADS, 0, ctx->stream>>>(A);
        SPK_HIP(hipGetLastError());
    }
    SPK_TRY(T.close());
    ctx->res_filter_ms = T.result();
    ctx->pl = std::move(npl);
    ctx->pr = std::move(npr);
    ctx->pvl = std::move(npvl);
    ctx->pvr = std::move(npvr);
    // pair_terms stays: every survivor still satisfies its rule's key terms.  The hidden pass leaves nothing a
    // later call could take for the caller's comparison vectors.
    ctx->pairs_replaced(n_out);
    ctx->set_rule_ranges(new_base, n_out);
    commit.done = true;
    if (out_n_pairs) *out_n_pairs = n_out;
    return SPK_OK;
}

namespace {
// spk_block_profile plans and enumerates under its own link type (plan_rule, build_by_position and enum_args read
// the context's) and hands the context's back on every way out.
struct LinkTypeLease {
    spk_ctx *ctx;
    int saved;
    LinkTypeLease(spk_ctx *c, int link_type) : ctx(c), saved(c->link_type) { c->link_type = link_type; }
    ~LinkTypeLease() { ctx->link_type = saved; }
};

// The first min(limit, B) blocks of a planned rule by descending metric into out[0 .. *n_out).  `bins`: blocks per
// bit length of the metric (k_block_stats).  With the cut, only the blocks in the bins >= j are sorted, j the highest
// bin with at least `limit` blocks at or above it (0 when the rule has fewer blocks).
int largest_blocks(spk_ctx *ctx, const RulePlan &P, int by_rows, const unsigned long long *bins, int limit,
                   spk_block_entry *out, int32_t *n_out, DevBuf<uint8_t> &tmp) {
    *n_out = 0;
    const int64_t B = P.B;
    if (B == 0 || limit == 0) return SPK_OK;
    int min_bin = 0;
    if (ctx->profile_cut) {
        unsigned long long above = 0;
        for (int j = SPK_PROFILE_BINS - 1; j > 0; --j) {
            above += bins[j];
            if (above >= (unsigned long long)limit) {
                min_bin = j;
                break;
            }
        }
    }
    CountScan pick;
    SPK_TRY(pick.alloc(ctx, B));
    const unsigned g = (unsigned)((B + 255) / 256);
    k_top_flag<<<g, 256, 0, ctx->stream>>>(B, P.cand.count.p, P.bstart.p, by_rows, min_bin, pick.count.p);
    SPK_HIP(hipGetLastError());
    SPK_TRY(scan_total(ctx, pick, tmp));
    const int64_t n = pick.total;
    SPK_REQUIRE(n >= std::min<int64_t>(limit, B) && n <= B, SPK_E_STATE, "spk_block_profile: largest-blocks cut");
    DevBuf<uint64_t> k_in, k_out;
    DevBuf<int32_t> i_in, i_out;
    SPK_TRY(k_in.alloc((size_t)n));
    SPK_TRY(k_out.alloc((size_t)n));
    SPK_TRY(i_in.alloc((size_t)n));
    SPK_TRY(i_out.alloc((size_t)n));
    k_top_emit<<<g, 256, 0, ctx->stream>>>(B, P.cand.count.p, P.bstart.p, by_rows, pick.count.p, pick.off.p, k_in.p,
                                           i_in.p);
    SPK_HIP(hipGetLastError());
    SPK_TRY(sort_pairs_u64(ctx->stream, tmp, k_in.p, k_out.p, i_in.p, i_out.p, n));
    const int m = (int)std::min<int64_t>(limit, n);
    DevBuf<spk_block_entry> d_out;
    SPK_TRY(d_out.alloc((size_t)m));
    k_top_entries<<<(unsigned)((m + 255) / 256), 256, 0, ctx->stream>>>(m, i_out.p, P.cand.count.p, P.bstart.p,
                                                                        P.bnR.p, P.tri, P.L.rows.p, d_out.p);
    SPK_HIP(hipGetLastError());
    SPK_HIP(hipMemcpyAsync(out, d_out.p, (size_t)m * sizeof(spk_block_entry), hipMemcpyDeviceToHost, ctx->stream));
    SPK_HIP(hipStreamSynchronize(ctx->stream));
    *n_out = m;
    return SPK_OK;
}

// Pairs spk_block's count pass keeps among the ordinals [lo, hi) of a rule whose by-position copies are built: one
// k_enum<false> launch per PROFILE_SLAB ordinals into the same chunk array, each reduced to one count on the device.
int count_ordinals(spk_ctx *ctx, const RulePlan &P, int64_t lo, int64_t hi, DevBuf<int64_t> &chunks,
                   DevBuf<uint8_t> &tmp, int64_t *out) {
    *out = 0;
    const int64_t n_slabs = (hi - lo + PROFILE_SLAB - 1) / PROFILE_SLAB;
    if (n_slabs <= 0) return SPK_OK;
    DevBuf<int64_t> d_sum;
    SPK_TRY(d_sum.alloc((size_t)n_slabs));
    SPK_TRY(chunks.alloc((size_t)(std::min(hi - lo, PROFILE_SLAB) + EN_CHUNK - 1) / EN_CHUNK));
    for (int64_t s = 0; s < n_slabs; ++s) {
        const int64_t q0 = lo + s * PROFILE_SLAB, q1 = std::min(q0 + PROFILE_SLAB, hi);
        const int64_t n_chunks = (q1 - q0 + EN_CHUNK - 1) / EN_CHUNK;
        EnumArgs A = enum_args(ctx, P, q0, q1);
        A.chunk_count = chunks.p;
        k_enum<false><<<(unsigned)n_chunks, EN_THREADS, 0, ctx->stream>>>(A);
        SPK_HIP(hipGetLastError());
        SPK_TRY(reduce_sum(ctx->stream, tmp, chunks.p, d_sum.p + s, n_chunks));
    }
    std::vector<int64_t> h((size_t)n_slabs);
    SPK_HIP(hipMemcpyAsync(h.data(), d_sum.p, (size_t)n_slabs * 8, hipMemcpyDeviceToHost, ctx->stream));
    SPK_HIP(hipStreamSynchronize(ctx->stream));
    for (int64_t v : h) *out += v;
    return SPK_OK;
}
}  // namespace

extern "C" int spk_block_profile(spk_ctx *ctx, int link_type, int n_rules, const int32_t *rule_symmetric,
                                 const int32_t *rule_program, int shard, int n_shards, int64_t max_enumerate,
                                 int largest_by, int limit, spk_rule_profile *out_rules, int64_t *out_hist,
                                 spk_block_entry *out_largest, int32_t *out_n_largest) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "null ctx");
    ctx->profile_ordinals = -1;
    ctx->profile_key_ms = ctx->profile_enum_ms = -1.0;
    SPK_REQUIRE(n_rules >= 1 && n_rules <= MAX_RULES && rule_symmetric && out_rules, SPK_E_INVALID,
                "spk_block_profile: need 1..32 rules");
    SPK_REQUIRE(link_type >= 0 && link_type <= 2, SPK_E_INVALID, "spk_block_profile: bad link_type");
    SPK_REQUIRE(n_shards >= 1 && shard >= 0 && shard < n_shards, SPK_E_INVALID, "spk_block_profile: bad shard");
    SPK_REQUIRE(largest_by == SPK_LARGEST_BY_CANDIDATES || largest_by == SPK_LARGEST_BY_ROWS_L, SPK_E_INVALID,
                "spk_block_profile: unknown largest_by");
    SPK_REQUIRE(limit >= 0, SPK_E_INVALID, "spk_block_profile: negative limit");
    SPK_REQUIRE(limit == 0 || (out_largest && out_n_largest), SPK_E_INVALID,
                "spk_block_profile: limit > 0 needs out_largest and out_n_largest");
    SPK_HIP(hipSetDevice(ctx->device));
    LinkTypeLease lease(ctx, link_type);
    Table &tl = ctx->table[0];
    Table &tr = ctx->side_table(1);
    SPK_REQUIRE(tl.n >= 0 && tr.n >= 0, SPK_E_STATE, "spk_block_profile: tables not loaded");
    const bool link_only = link_type == SPK_LINK_ONLY;
    SPK_REQUIRE(link_only || tl.rank.p || tl.n == 0, SPK_E_STATE, "spk_block_profile: rank not set");
    for (int r = 0; r < n_rules; ++r) {
        SPK_REQUIRE((int)tl.key[0].size() > r && tl.key[0][r]->p && (int)tr.key[1].size() > r && tr.key[1][r]->p,
                    SPK_E_STATE, "spk_block_profile: keys not set for every rule");
    }
    // ---- key level: per rule the plan (sorted views, blocks, candidates per block and their scan), the block
    // statistics and the largest blocks.  A plan is kept only while its rule may still be enumerated.
    StageTimer key_t{ctx}, enum_t{ctx};  // two readings, one after the other
    DevBuf<uint8_t> tmp;
    DevBuf<ProfileStats> d_stats;
    SPK_TRY(d_stats.alloc(1));
    std::vector<RulePlan> plans(n_rules);
    int64_t total = 0;
    SPK_TRY(key_t.open());
    for (int r = 0; r < n_rules; ++r) {
        RulePlan &P = plans[r];
        SPK_TRY(plan_rule(ctx, r, rule_symmetric[r] != 0, P, tmp));
        ProfileStats st;
        std::memset(&st, 0, sizeof(st));
        if (P.B > 0) {
            SPK_HIP(hipMemsetAsync(d_stats.p, 0, sizeof(ProfileStats), ctx->stream));
            const unsigned g = (unsigned)std::min<int64_t>((P.B + PS_THREADS - 1) / PS_THREADS, 4 * (int64_t)ctx->n_cu);
            k_block_stats<<<g, PS_THREADS, 0, ctx->stream>>>(P.B, P.cand.count.p, P.bstart.p, d_stats.p);
            SPK_HIP(hipGetLastError());
            SPK_HIP(hipMemcpyAsync(&st, d_stats.p, sizeof(st), hipMemcpyDeviceToHost, ctx->stream));
            SPK_HIP(hipStreamSynchronize(ctx->stream));
        }
        spk_rule_profile &o = out_rules[r];
        o.rows_l = P.L.n_valid;
        o.rows_r = P.tri ? P.L.n_valid : P.R.n_valid;
        o.blocks = P.B;
        o.candidates = P.cand.total;
        o.largest_candidates = (int64_t)st.largest;
        o.enumerated = -1;
        total += P.cand.total;
        if (out_hist)
            for (int i = 0; i < SPK_PROFILE_BINS; ++i) {
                out_hist[((size_t)r * SPK_PROFILE_BINS + i) * 2 + 0] = (int64_t)st.hist[i][0];
                out_hist[((size_t)r * SPK_PROFILE_BINS + i) * 2 + 1] = (int64_t)st.hist[i][1];
            }
        if (limit > 0) {
            const bool by_rows = largest_by == SPK_LARGEST_BY_ROWS_L;
            unsigned long long bins[SPK_PROFILE_BINS];
            for (int i = 0; i < SPK_PROFILE_BINS; ++i) bins[i] = by_rows ? st.rows_bins[i] : st.hist[i][0];
            SPK_TRY(largest_blocks(ctx, P, by_rows ? 1 : 0, bins, limit, out_largest + (size_t)r * limit,
                                   out_n_largest + r, tmp));
        }
        if (max_enumerate == 0) P = RulePlan();
    }
    if (ctx->timing) SPK_TRY(key_t.close());  // timing off: nothing here waits for the stream
    // ---- enumeration: this shard's ordinals of each rule, cut as block_rules cuts them
    const int64_t g_lo = (int64_t)((__int128)total * shard / n_shards);
    const int64_t g_hi = (int64_t)((__int128)total * (shard + 1) / n_shards);
    int64_t acc = 0, ordinals = 0;
    DevBuf<int64_t> chunks;
    SPK_TRY(enum_t.open());
    for (int r = 0; r < n_rules && max_enumerate != 0; ++r) {
        RulePlan &P = plans[r];
        const int64_t lo = std::max<int64_t>(g_lo - acc, 0), hi = std::min<int64_t>(g_hi - acc, P.cand.total);
        acc += P.cand.total;
        const int64_t len = std::max<int64_t>(hi - lo, 0);
        if (max_enumerate > 0 && len > max_enumerate) {
            P = RulePlan();
            continue;
        }
        if (len > 0) {
            std::vector<int> excl;
            for (int j = 0; j < r; ++j)
                if (!rule_program || rule_program[j] < 0) excl.push_back(j);
            SPK_TRY(build_by_position(ctx, excl, P));
            SPK_TRY(count_ordinals(ctx, P, lo, hi, chunks, tmp, &out_rules[r].enumerated));
            ordinals += len;
        } else {
            out_rules[r].enumerated = 0;
        }
        P = RulePlan();  // the rule's views, blocks and by-position copies
    }
    if (ctx->timing) SPK_TRY(enum_t.close());
    ctx->profile_key_ms = key_t.result();
    ctx->profile_enum_ms = enum_t.result();
    ctx->profile_ordinals = ordinals;
    return SPK_OK;
}

extern "C" int spk_block_profile_info(spk_ctx *ctx, double *out_key_ms, double *out_enum_ms,
                                      int64_t *out_ordinals_enumerated) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "null ctx");
    if (out_key_ms) *out_key_ms = ctx->profile_key_ms;
    if (out_enum_ms) *out_enum_ms = ctx->profile_enum_ms;
    if (out_ordinals_enumerated) *out_ordinals_enumerated = ctx->profile_ordinals;
    return SPK_OK;
}

extern "C" int spk_block_profile_set_cut(spk_ctx *ctx, int on) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "null ctx");
    ctx->profile_cut = on != 0;
    return SPK_OK;
}

extern "C" int spk_block_residual_info(spk_ctx *ctx, int64_t *out_enumerated, double *out_filter_ms) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "null ctx");
    if (out_enumerated) *out_enumerated = ctx->res_enumerated;
    if (out_filter_ms) *out_filter_ms = ctx->res_filter_ms;
    return SPK_OK;
}
