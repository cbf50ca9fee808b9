// Best match per record (gfx950): df_e.filter(...).best_matches(per=...) on the device.
//
// S = the survivors of the context's selection whose score is not NULL (NaN); the score is match_probability (the
// selection's own per-pattern table) or tf_adjusted_match_prob (its tf_mp).  Pair a beats pair b iff score(a) >
// score(b), or the scores are equal as doubles and ordinal(a) < ordinal(b): a strict total order, so "the pair that
// beats every other pair of its group" names one pair whatever the algorithm, the launch shape or the order in which
// atomics arrive, and two runs agree bit for bit.  A group is the pairs that share a record: by left record
// (SPK_BEST_L), by right record (SPK_BEST_R), or the pairs touching a record on either side (SPK_BEST_EITHER keeps a
// pair that is the best of its left or of its right record, SPK_BEST_MUTUAL one that is the best of both).  With
// keep_ties every pair whose score equals its group's maximum counts as a best pair of the group.
//
// Records are named by their table rows (a table's permutation is a bijection, so rows serve as group ids as well as
// input positions would); link_only offsets the right table's rows by the left table's row count, the other link
// types index table 0 on both sides.  Four launches over the survivors, in the chunk layout of spk_select (one wave
// per chunk of BEST_CHUNK survivors, 64 consecutive survivors per slab, a capped grid striding over the chunks):
//   k_best_max    per group an unsigned 64-bit atomic max of an order-preserving image of the fp64 score;
//   k_best_first  (not with keep_ties) among the pairs whose image equals their group's max, a 64-bit atomic min of
//                 the survivor index: the selection is in ascending ordinal, so the smallest index is the smallest
//                 ordinal;
//   k_best_keep   the keep flag of every survivor as one ballot word per slab, and the kept pairs per chunk;
//   k_best_emit   after the scan of the counts (CountScan): the kept pairs' ordinal, rows, code and, when the
//                 selection has them, tf_adjusted_match_prob and the adjustment rows, into buffers of the kept count,
//                 in the order of the survivors.
// No workgroup waits for another inside a launch: no spin, no ticket, no cooperative launch, and every loop has a
// fixed bound.  Every pass checks a pair's rows against the tables before it indexes a group array with them; a row
// outside its table (never written by this library) is reported by k_best_max and the call fails.
//
// Contention: a record in 20,000 pairs puts 20,000 updates on one word.  Before an atomic the word is read past the
// L1 (an agent-scope load) and the atomic is left out when it cannot improve the word (cc_lower's form,
// spk_components.hip).  k_enum emits a block's pairs with the left row non-decreasing, so survivors of one left
// record sit in neighbouring lanes: in the COLLAPSE form a wave-level segmented max over the lanes' left rows leaves
// one atomic per run of equal left rows (and k_best_first leaves out a candidate whose lower neighbour is a candidate
// of the same record).  The right side has no such order and takes the plain form.  A/B of the two forms on MI355X,
// mode by mode (the collapse won under SPK_BEST_L only, and runs there): profiles/ab_best_matches.log, DESIGN.md.
#include <algorithm>

#include "spk_prim.h"

// One atomic per run of equal left rows in a wave (the COLLAPSE form of k_best_max / k_best_first): 0 never (one atomic
// per pair), 1 under SPK_BEST_L only, 2 under every mode with left groups.  1 is what won on MI355X mode by mode
// (tools/ab_best.py, profiles/ab_best_matches.log).
#ifndef SPK_BEST_COLLAPSE
#define SPK_BEST_COLLAPSE 1
#endif

namespace spk {

constexpr int BEST_THREADS = 256;
constexpr int BEST_WAVES = BEST_THREADS / 64;
constexpr int64_t BEST_CHUNK = 2048;               // survivors per count: spk_select's SEL_CHUNK (_native.SELECT_CHUNK)
constexpr int BEST_SLABS = (int)(BEST_CHUNK / 64);  // ballot words per chunk
constexpr int BEST_WG_PER_CU = 8;                  // capped grid, the waves stride over the chunks (as k_select)

struct BestArgs {
    int64_t n, n_chunks;          // survivors, chunks of BEST_CHUNK
    const int64_t *ord;
    const int32_t *l, *r;
    const uint32_t *code;
    const double *mpat;           // SPK_SEL_MP: score = mpat[code] ...
    int64_t n_pat;
    const double *tf_mp;          // ... SPK_SEL_TF_MP: score = tf_mp[i] (mpat is then null)
    const double *adj;            // [n x n_tf] or null
    int n_tf;
    int64_t n0, n1;               // rows of the l / r side's table
    int64_t r_base;               // group id of the r side's row 0 (link_only: n0)
    int mode, keep_ties;
    unsigned long long *gmax;     // [n_groups] the largest score image of the group, 0 = none
    unsigned long long *gwin;     // [n_groups] the smallest survivor index among the group's maxima (not keep_ties)
    unsigned int *bad;            // a pair names a row outside its table
    unsigned long long *bitmap;   // [n_chunks x BEST_SLABS] keep ballots
    int64_t *chunk_count;         // [n_chunks]
    const int64_t *chunk_off;     // [n_chunks + 1]
    int64_t *out_ord;
    int32_t *out_l, *out_r;
    uint32_t *out_code;
    double *out_tf, *out_adj;
};

// Order-preserving image of a score: a < b as doubles iff image(a) < image(b) as unsigned, for every non-NaN value
// (-inf .. +inf, subnormals included; -0.0 and +0.0, equal as doubles, share one image).  No value maps to 0, which
// stands for "no score" (NaN = NULL): such a pair is never kept and never beats anything.
__device__ inline unsigned long long best_image(double s) {
    if (s != s) return 0ull;
    unsigned long long u = (unsigned long long)__double_as_longlong(s);
    if ((u << 1) == 0ull) u = 0ull;  // -0.0 -> +0.0
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

// One survivor as the passes see it: its group ids (-1: that side takes no part) and its score image (0: NULL, a row
// outside its table, or past the end).
struct BestPair {
    int64_t gl, gr;
    unsigned long long img;
    bool bad;
};

__device__ inline BestPair best_pair(const BestArgs &A, int64_t i) {
    BestPair p{-1, -1, 0ull, false};
    if (i >= A.n) return p;
    const int64_t l = A.l[i], r = A.r[i];
    if (l < 0 || l >= A.n0 || r < 0 || r >= A.n1) {
        p.bad = true;
        return p;
    }
    double s;
    if (A.tf_mp) {
        s = A.tf_mp[i];
    } else {
        const int64_t c = A.code[i];
        if (c >= A.n_pat) {  // spk_select kept no such code
            p.bad = true;
            return p;
        }
        s = A.mpat[c];
    }
    p.img = best_image(s);
    if (p.img == 0ull) return p;
    if (A.mode != SPK_BEST_R) p.gl = l;
    if (A.mode != SPK_BEST_L) p.gr = A.r_base + r;
    return p;
}

__device__ inline void best_raise(unsigned long long *w, unsigned long long to) {
    if (__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < to)
        (void)__hip_atomic_fetch_max(w, to, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ inline void best_lower(unsigned long long *w, unsigned long long to) {
    if (__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > to)
        (void)__hip_atomic_fetch_min(w, to, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Pass (a).  COLLAPSE: an inclusive segmented max over the lanes by left group id (six shuffle steps; a lane joins
// the value of the lane `off` below it when that lane has its group id, so every value stays a score of the lane's
// own group), and only the last lane of every run of equal ids issues the atomic, with the run's maximum.
template <bool COLLAPSE>
__global__ __launch_bounds__(BEST_THREADS) void k_best_max(BestArgs A) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n_waves = (int64_t)gridDim.x * BEST_WAVES;
    bool bad = false;
    for (int64_t c = (int64_t)blockIdx.x * BEST_WAVES + wave; c < A.n_chunks; c += n_waves) {
        const int64_t base = c * BEST_CHUNK;
        for (int s = 0; s < BEST_SLABS; ++s) {
            const int64_t i0 = base + (int64_t)s * 64;
            if (i0 >= A.n) break;  // wave-uniform
            const BestPair p = best_pair(A, i0 + lane);
            bad = bad || p.bad;
            if (COLLAPSE) {
                unsigned long long v = p.gl >= 0 ? p.img : 0ull;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const unsigned long long ov = __shfl_up(v, off, 64);
                    const long long og = __shfl_up((long long)p.gl, off, 64);
                    if (lane >= off && og == (long long)p.gl && ov > v) v = ov;
                }
                const long long ng = __shfl_down((long long)p.gl, 1, 64);
                const bool tail = lane == 63 || ng != (long long)p.gl;
                if (p.gl >= 0 && tail) best_raise(A.gmax + p.gl, v);
            } else if (p.gl >= 0) {
                best_raise(A.gmax + p.gl, p.img);
            }
            if (p.gr >= 0) best_raise(A.gmax + p.gr, p.img);
        }
    }
    if (__ballot(bad) != 0ull && lane == 0) (void)__hip_atomic_fetch_or(A.bad, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Pass (b).  The maxima are final (the launch before this one wrote them).  COLLAPSE: a candidate whose lower
// neighbour lane is a candidate of the same left record has the larger index and issues nothing.
template <bool COLLAPSE>
__global__ __launch_bounds__(BEST_THREADS) void k_best_first(BestArgs A) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n_waves = (int64_t)gridDim.x * BEST_WAVES;
    for (int64_t c = (int64_t)blockIdx.x * BEST_WAVES + wave; c < A.n_chunks; c += n_waves) {
        const int64_t base = c * BEST_CHUNK;
        for (int s = 0; s < BEST_SLABS; ++s) {
            const int64_t i0 = base + (int64_t)s * 64;
            if (i0 >= A.n) break;  // wave-uniform
            const int64_t i = i0 + lane;
            const BestPair p = best_pair(A, i);
            bool cl = p.gl >= 0 && A.gmax[p.gl] == p.img;
            const bool cr = p.gr >= 0 && A.gmax[p.gr] == p.img;
            if (COLLAPSE) {
                const long long cand = cl ? (long long)p.gl : -1ll;
                const long long below = __shfl_up(cand, 1, 64);
                if (lane > 0 && cl && below == cand) cl = false;
            }
            if (cl) best_lower(A.gwin + p.gl, (unsigned long long)i);
            if (cr) best_lower(A.gwin + p.gr, (unsigned long long)i);
        }
    }
}

// Pass (c): is survivor i kept?  One ballot word per slab and the chunk's count.
__global__ __launch_bounds__(BEST_THREADS) void k_best_keep(BestArgs A) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n_waves = (int64_t)gridDim.x * BEST_WAVES;
    for (int64_t c = (int64_t)blockIdx.x * BEST_WAVES + wave; c < A.n_chunks; c += n_waves) {
        const int64_t base = c * BEST_CHUNK;
        int total = 0;
        for (int s = 0; s < BEST_SLABS; ++s) {
            const int64_t i = base + (int64_t)s * 64 + lane;
            const BestPair p = best_pair(A, i);  // past the end: no group, not kept
            bool bl = false, br = false;
            if (A.keep_ties) {
                bl = p.gl >= 0 && A.gmax[p.gl] == p.img;
                br = p.gr >= 0 && A.gmax[p.gr] == p.img;
            } else {
                bl = p.gl >= 0 && A.gwin[p.gl] == (unsigned long long)i;
                br = p.gr >= 0 && A.gwin[p.gr] == (unsigned long long)i;
            }
            const bool k = A.mode == SPK_BEST_MUTUAL ? (bl && br) : (bl || br);
            const unsigned long long w = __ballot(k);
            total += __popcll(w);
            if (lane == 0) A.bitmap[c * BEST_SLABS + s] = w;
        }
        if (lane == 0) A.chunk_count[c] = total;
    }
}

// Pass (d): the kept pairs at chunk offset + kept pairs before them, the order of the survivors.
__global__ __launch_bounds__(BEST_THREADS) void k_best_emit(BestArgs A) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int64_t n_waves = (int64_t)gridDim.x * BEST_WAVES;
    for (int64_t c = (int64_t)blockIdx.x * BEST_WAVES + wave; c < A.n_chunks; c += n_waves) {
        int64_t run = A.chunk_off[c];
        if (A.chunk_off[c + 1] == run) continue;  // nothing kept here (wave-uniform)
        const int64_t base = c * BEST_CHUNK;
        for (int s = 0; s < BEST_SLABS; ++s) {
            const unsigned long long w = A.bitmap[c * BEST_SLABS + s];
            if ((w >> lane) & 1ull) {  // a kept pair lies below n (k_best_keep)
                const int64_t i = base + (int64_t)s * 64 + lane;
                const int64_t q = run + __popcll(w & below);
                A.out_ord[q] = A.ord[i];
                A.out_l[q] = A.l[i];
                A.out_r[q] = A.r[i];
                A.out_code[q] = A.code[i];
                if (A.out_tf) A.out_tf[q] = A.tf_mp[i];
                if (A.out_adj)
                    for (int t = 0; t < A.n_tf; ++t) A.out_adj[q * A.n_tf + t] = A.adj[i * A.n_tf + t];
            }
            run += __popcll(w);
        }
    }
}

static unsigned best_grid(const spk_ctx *ctx, int64_t n_chunks) {
    const int64_t g = (n_chunks + BEST_WAVES - 1) / BEST_WAVES;
    return (unsigned)std::max<int64_t>(std::min<int64_t>(g, BEST_WG_PER_CU * (int64_t)ctx->n_cu), 1);
}

// The narrowing of S (the context's former selection, now a local of spk_select_best) into T.
static int narrow_selection(spk_ctx *ctx, Selection &S, int field, int mode, int keep_ties, const NodeSpace &N,
                            Selection &T, double &ms_out) {
    const int64_t n_groups = N.n_nodes;
    hipStream_t st = ctx->stream;
    const int64_t n = S.n;
    T.K = S.K;
    T.n_levels = S.n_levels;
    T.stride = S.stride;
    T.has_rows = true;
    T.has_mp = S.has_mp;
    T.has_tf = S.has_tf;
    T.n_tf = S.n_tf;
    T.pairs_epoch = S.pairs_epoch;
    T.gamma_seq = S.gamma_seq;
    T.fix_seq = S.fix_seq;
    T.ms = S.ms;  // spk_select_info keeps its meaning: the time of the selection's own kernels
    StageTimer watch{ctx};
    int64_t kept = 0;
    const int64_t n_chunks = (n + BEST_CHUNK - 1) / BEST_CHUNK;
    BestArgs A{};
    DevBuf<unsigned long long> gmax, gwin, bitmap;  // temporaries: gone at return
    DevBuf<unsigned int> bad;
    DevBuf<uint8_t> tmp;
    CountScan chunks;
    if (n > 0) {
        SPK_TRY(gmax.alloc((size_t)n_groups + 1));
        if (!keep_ties) SPK_TRY(gwin.alloc((size_t)n_groups + 1));
        SPK_TRY(bitmap.alloc((size_t)(n_chunks * BEST_SLABS) + 1));
        SPK_TRY(bad.alloc(1));
        SPK_TRY(chunks.alloc(ctx, n_chunks));
        A.n = n;
        A.n_chunks = n_chunks;
        A.ord = S.ord.p;
        A.l = S.l.p;
        A.r = S.r.p;
        A.code = S.code.p;
        A.mpat = field == SPK_SEL_MP ? S.mpat.p : nullptr;
        A.n_pat = field == SPK_SEL_MP ? (int64_t)S.mpat.n - 1 : 0;  // build_selection allocates n_patterns + 1
        A.tf_mp = field == SPK_SEL_TF_MP ? S.tf_mp.p : nullptr;
        A.n_tf = S.n_tf;
        A.n0 = N.n0;
        A.n1 = N.n1;
        A.r_base = N.r_base;
        A.mode = mode;
        A.keep_ties = keep_ties;
        A.gmax = gmax.p;
        A.gwin = gwin.p;
        A.bad = bad.p;
        A.bitmap = bitmap.p;
        A.chunk_count = chunks.count.p;
        const unsigned g = best_grid(ctx, n_chunks);
        SPK_TRY(watch.open());
        SPK_HIP(hipMemsetAsync(gmax.p, 0, ((size_t)n_groups + 1) * 8, st));
        if (!keep_ties) SPK_HIP(hipMemsetAsync(gwin.p, 0xFF, ((size_t)n_groups + 1) * 8, st));  // no winner yet
        SPK_HIP(hipMemsetAsync(bad.p, 0, sizeof(unsigned int), st));
        const bool collapse = SPK_BEST_COLLAPSE == 2 ? mode != SPK_BEST_R : SPK_BEST_COLLAPSE == 1 && mode == SPK_BEST_L;
        if (collapse) k_best_max<true><<<g, BEST_THREADS, 0, st>>>(A);
        else k_best_max<false><<<g, BEST_THREADS, 0, st>>>(A);
        SPK_HIP(hipGetLastError());
        if (!keep_ties) {
            if (collapse) k_best_first<true><<<g, BEST_THREADS, 0, st>>>(A);
            else k_best_first<false><<<g, BEST_THREADS, 0, st>>>(A);
            SPK_HIP(hipGetLastError());
        }
        k_best_keep<<<g, BEST_THREADS, 0, st>>>(A);
        SPK_HIP(hipGetLastError());
        unsigned int h_bad = 0u;
        SPK_HIP(hipMemcpyAsync(&h_bad, bad.p, sizeof(h_bad), hipMemcpyDeviceToHost, st));
        SPK_TRY(scan_total(ctx, chunks, tmp, &watch));  // synchronises
        SPK_REQUIRE(h_bad == 0u, SPK_E_STATE, "spk_select_best: a selected pair names a row outside its table");
        kept = chunks.total;
        SPK_REQUIRE(kept >= 0 && kept <= n, SPK_E_STATE, "spk_select_best: kept count");
    }
    SPK_TRY(T.ord.alloc((size_t)kept + 1));
    SPK_TRY(T.code.alloc((size_t)kept + 1));
    SPK_TRY(T.l.alloc((size_t)kept + 1));
    SPK_TRY(T.r.alloc((size_t)kept + 1));
    if (S.has_tf) {
        SPK_TRY(T.tf_mp.alloc((size_t)kept + 1));
        SPK_TRY(T.adj.alloc((size_t)kept * S.n_tf + 1));
    }
    if (kept > 0) {
        A.chunk_count = nullptr;
        A.chunk_off = chunks.off.p;
        A.out_ord = T.ord.p;
        A.out_l = T.l.p;
        A.out_r = T.r.p;
        A.out_code = T.code.p;
        if (S.has_tf) {
            A.tf_mp = S.tf_mp.p;  // copied whichever field scored
            A.adj = S.adj.p;
            A.out_tf = T.tf_mp.p;
            A.out_adj = S.n_tf > 0 ? T.adj.p : nullptr;
        }
        SPK_TRY(watch.open());
        k_best_emit<<<best_grid(ctx, n_chunks), BEST_THREADS, 0, st>>>(A);
        SPK_HIP(hipGetLastError());
        SPK_TRY(watch.close());
    }
    T.mpat = std::move(S.mpat);
    T.n = kept;
    T.valid = true;
    ms_out = watch.result();
    return SPK_OK;
}

}  // namespace spk

using namespace spk;

extern "C" int spk_select_best(spk_ctx *ctx, int field, int mode, int keep_ties, int64_t *out_n_kept) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "spk_select_best: null ctx");
    SPK_HIP(hipSetDevice(ctx->device));
    Selection S = std::move(ctx->sel);  // freed when this call returns, whatever happens below ...
    ctx->sel.clear();                   // ... and a failing call leaves no selection
    ctx->best_before = ctx->best_kept = -1;
    ctx->best_ms = -1.0;
    SPK_REQUIRE(field == SPK_SEL_MP || field == SPK_SEL_TF_MP, SPK_E_INVALID,
                "spk_select_best: unknown field (SPK_SEL_MP or SPK_SEL_TF_MP)");
    SPK_REQUIRE(mode >= SPK_BEST_L && mode <= SPK_BEST_MUTUAL, SPK_E_INVALID,
                "spk_select_best: unknown mode (SPK_BEST_L, _R, _EITHER or _MUTUAL)");
    SPK_REQUIRE(keep_ties == 0 || keep_ties == 1, SPK_E_INVALID, "spk_select_best: keep_ties is 0 or 1");
    SPK_REQUIRE(S.valid, SPK_E_STATE, "spk_select_best: no selection (run spk_select)");
    SPK_REQUIRE(S.current(ctx), SPK_E_STATE, "spk_select_best: the pairs or codes changed since spk_select");
    SPK_REQUIRE(S.has_rows, SPK_E_STATE, "spk_select_best: no pair rows (a loaded gamma table)");
    SPK_REQUIRE(field != SPK_SEL_MP || S.has_mp, SPK_E_STATE,
                "spk_select_best: no match_probability (spk_select got no m / u)");
    SPK_REQUIRE(field != SPK_SEL_TF_MP || S.has_tf, SPK_E_STATE,
                "spk_select_best: no tf_adjusted_match_prob (the selection was made without tf tables, spk_select)");
    const NodeSpace N = node_space(ctx);
    SPK_REQUIRE(N.n0 >= 0 && N.n1 >= 0, SPK_E_STATE, "spk_select_best: no tables");
    Selection T;
    double ms = -1.0;
    SPK_TRY(narrow_selection(ctx, S, field, mode, keep_ties, N, T, ms));
    ctx->best_before = S.n;
    ctx->best_kept = T.n;
    ctx->best_ms = ms;
    ctx->sel = std::move(T);
    if (out_n_kept) *out_n_kept = ctx->sel.n;
    return SPK_OK;
}

extern "C" int spk_select_best_info(spk_ctx *ctx, int64_t *out_n_before, int64_t *out_n_kept, double *out_ms) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "spk_select_best_info: null ctx");
    if (out_n_before) *out_n_before = ctx->best_before;
    if (out_n_kept) *out_n_kept = ctx->best_kept;
    if (out_ms) *out_ms = ctx->best_ms;
    return SPK_OK;
}
