// Connected components of the kept pairs (gfx950): df_e.filter(...).clusters() on the device.
//
// label[v] = the smallest node id of v's component; a node without edges keeps label[v] = v.  That definition does
// not depend on the algorithm, the edge order, the launch shape or the order in which atomics arrive, so two runs
// agree bit for bit.  Node ids are input positions: k_cc_edges takes the selection's rows through the tables'
// permutations once, and every round then streams 8 bytes per edge.
//
// Min-label hooking with pointer jumping, a host-driven loop of rounds.  One round is two launches:
//   k_cc_hook  per edge (u, v): climb from label[u] and from label[v] (label of label, at most CC_CLIMB loads, ends
//              at a root x = label[x]); if the two ends differ, lower the larger one's label to the smaller one;
//   k_cc_jump  per node v: climb from label[v]; if that ends below label[v], lower label[v] to it.
// The loop ends after the first round in which no edge had different ends and no label was lowered; the host reads
// that word after the round's launches have completed.  No workgroup waits for another inside a launch: there is no
// spin, no ticket and no cooperative launch, and every loop in a kernel has a fixed bound, so nothing here can hang.
//
// The 8 XCDs have private L2s and a CU's L1 is never refreshed by another CU's writes, so a plain load of a label
// that another workgroup lowered in the same launch may return the older value.  Two invariants make that harmless:
//   (1) a label only ever decreases:        it is written by k_cc_init (plain stores, label[v] = v, a launch in which
//                                           nothing else touches the word) and after that only by agent-scope atomic
//                                           minima;
//   (2) label[v] is an id of v's component: v itself at first, and every minimum stores a value reached by climbing
//                                           from an endpoint of an edge of that component (hook) or from v (jump).
// By (1) a stale value is a larger former label, which by (2) is still an id of the same component and still
// satisfies label[x] <= x: climbing over stale values ends at some member of the component, and the minimum it feeds
// is legal.  A stale read can therefore cost a round, never correctness.  The round that ends the loop wrote
// nothing, so every load in it saw the final array: all edges then join nodes with one common label, every label is a
// root, a root is <= every node that carries it, and so it is the component's smallest id.
//
// Contention (a record duplicated 1,000 times is a clique hooking into one root): an edge whose endpoints carry the
// same label is skipped after two loads, and before the atomic the target word is read again past the L1 (an
// agent-scope load) and the atomic is left out when the word is already as low.  Rounds on the test graphs, emulated
// on the host with every load as stale as it can be (tools/emulate_components.py): DESIGN.md.
#include <algorithm>

#include "spk_internal.h"

namespace spk {

constexpr int CC_THREADS = 256;
constexpr int CC_VEC = 4;                                 // edges per lane and chunk: one 16-byte load of u, one of v
constexpr int64_t CC_CHUNK = (int64_t)CC_THREADS * CC_VEC;  // edges per workgroup step; _native.COMPONENTS_CHUNK mirrors it
constexpr int CC_WG_PER_CU = 8;                           // capped grid, the workgroups stride over the chunks (as k_select)
constexpr int CC_CLIMB = 8;                               // loads of one climb; tools/emulate_components.py mirrors it
constexpr int CC_MAX_ROUNDS = 256;                        // the loop's hard cap (SPK_E_LIMIT beyond it)

typedef uint32_t cc_u32x4 __attribute__((ext_vector_type(4)));

__device__ inline uint32_t cc_load(uint32_t *label, uint32_t x) { return label[(size_t)x]; }

// From r (a label already loaded) upwards: at most CC_CLIMB - 1 more loads, ends at the first x with label[x] == x.
__device__ inline uint32_t cc_climb(uint32_t *label, uint32_t r) {
    for (int s = 1; s < CC_CLIMB; ++s) {
        const uint32_t up = cc_load(label, r);
        if (up == r) break;
        r = up;
    }
    return r;
}

__device__ inline void cc_lower(uint32_t *label, uint32_t x, uint32_t to) {
    uint32_t *w = label + (size_t)x;
    if (__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > to)
        (void)__hip_atomic_fetch_min(w, to, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// flags[0]: this round is not quiet; flags[1]: an edge named a node >= n_nodes (CHECK launches)
__device__ inline void cc_raise(unsigned int *flags, bool changed, bool bad) {
    const bool any_c = __ballot(changed) != 0ull, any_b = __ballot(bad) != 0ull;
    if ((threadIdx.x & 63) == 0) {
        if (any_c) (void)__hip_atomic_fetch_or(flags, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (any_b) (void)__hip_atomic_fetch_or(flags + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(CC_THREADS) void k_cc_init(int64_t n_nodes, uint32_t *__restrict__ label) {
    const int64_t step = (int64_t)gridDim.x * CC_THREADS;
    for (int64_t v = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x; v < n_nodes; v += step) label[v] = (uint32_t)v;
}

struct EdgeArgs {
    int64_t n_edges;
    const int32_t *l, *r;          // the selection's rows
    const int32_t *perm0, *perm1;  // table row -> input row of the l / r side's table, or null (identity)
    int64_t n0, n1;                // rows of the l / r side's table
    uint32_t r_base;               // node id of the r side's input row 0 (link_only: n0)
    uint32_t *u, *v;
};

// The selection's pairs as node ids.  A row outside its table (never written by this library) becomes id 2^32 - 1,
// which no graph has (n_nodes <= 2^32 - 1), so the first hook launch reports it and no permutation is read for it.
__global__ __launch_bounds__(CC_THREADS) void k_cc_edges(EdgeArgs A) {
    const int64_t step = (int64_t)gridDim.x * CC_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x; i < A.n_edges; i += step) {
        const int64_t l = A.l[i], r = A.r[i];
        uint32_t u = 0xFFFFFFFFu, v = 0xFFFFFFFFu;
        if (l >= 0 && l < A.n0) u = (uint32_t)(A.perm0 ? A.perm0[l] : (int32_t)l);
        if (r >= 0 && r < A.n1) v = A.r_base + (uint32_t)(A.perm1 ? A.perm1[r] : (int32_t)r);
        A.u[i] = u;
        A.v[i] = v;
    }
}

template <bool CHECK>
__device__ inline void cc_hook_edge(uint32_t *label, int64_t n_nodes, uint32_t u, uint32_t v, bool &changed, bool &bad) {
    if (CHECK && ((int64_t)u >= n_nodes || (int64_t)v >= n_nodes)) {
        bad = true;
        return;
    }
    if (u == v) return;
    uint32_t a = cc_load(label, u), b = cc_load(label, v);
    if (a == b) return;
    a = cc_climb(label, a);
    b = cc_climb(label, b);
    if (a == b) return;  // one tree, not flat yet: k_cc_jump lowers a label in it and reports that
    changed = true;
    cc_lower(label, a > b ? a : b, a > b ? b : a);
}

// CHECK: the first round's launch, which validates every id before it indexes the labels with it.
template <bool CHECK>
__global__ __launch_bounds__(CC_THREADS) void k_cc_hook(int64_t n_nodes, int64_t n_edges, const uint32_t *__restrict__ eu,
                                                        const uint32_t *__restrict__ ev, uint32_t *label,
                                                        unsigned int *flags) {
    bool changed = false, bad = false;
    const int64_t n_chunks = (n_edges + CC_CHUNK - 1) / CC_CHUNK;
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const int64_t e0 = c * CC_CHUNK + (int64_t)threadIdx.x * CC_VEC;
        if (e0 + CC_VEC <= n_edges) {  // the buffers start 256-byte aligned and e0 is a multiple of 4
            const cc_u32x4 uu = __builtin_nontemporal_load(reinterpret_cast<const cc_u32x4 *>(eu + e0));
            const cc_u32x4 vv = __builtin_nontemporal_load(reinterpret_cast<const cc_u32x4 *>(ev + e0));
#pragma unroll
            for (int j = 0; j < CC_VEC; ++j) cc_hook_edge<CHECK>(label, n_nodes, uu[j], vv[j], changed, bad);
        } else {
            for (int j = 0; j < CC_VEC; ++j)
                if (e0 + j < n_edges) cc_hook_edge<CHECK>(label, n_nodes, eu[e0 + j], ev[e0 + j], changed, bad);
        }
    }
    cc_raise(flags, changed, bad);
}

__global__ __launch_bounds__(CC_THREADS) void k_cc_jump(int64_t n_nodes, uint32_t *label, unsigned int *flags) {
    bool changed = false;
    const int64_t step = (int64_t)gridDim.x * CC_THREADS;
    for (int64_t v = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x; v < n_nodes; v += step) {
        const uint32_t p = label[v];
        if ((int64_t)p == v) continue;
        const uint32_t r = cc_climb(label, p);
        if (r < p) {
            changed = true;
            (void)__hip_atomic_fetch_min(label + v, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    cc_raise(flags, changed, false);
}

// *count += the nodes that are their own label (one add per wave)
__global__ __launch_bounds__(CC_THREADS) void k_cc_count(int64_t n_nodes, const uint32_t *__restrict__ label,
                                                         unsigned long long *count) {
    unsigned long long mine = 0;
    const int64_t step = (int64_t)gridDim.x * CC_THREADS;
    for (int64_t v = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x; v < n_nodes; v += step)
        mine += (int64_t)label[v] == v ? 1ull : 0ull;
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_down(mine, off, 64);
    if ((threadIdx.x & 63) == 0 && mine)
        (void)__hip_atomic_fetch_add(count, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

static unsigned cc_grid(const spk_ctx *ctx, int64_t items, int64_t per_wg) {
    const int64_t g = (items + per_wg - 1) / per_wg;
    return (unsigned)std::max<int64_t>(std::min<int64_t>(g, CC_WG_PER_CU * (int64_t)ctx->n_cu), 1);
}

// Labels of the graph (eu, ev) [n_edges] over n_nodes nodes into C, a local of the caller.  `first` is an event pair
// already open around the caller's own launches (the edge build), or false.
static int build_components(spk_ctx *ctx, int64_t n_nodes, int64_t n_edges, const uint32_t *eu, const uint32_t *ev,
                            int bad_code, const char *bad_msg, bool first, Components &C) {
    hipStream_t st = ctx->stream;
    double ms = 0.0;
    auto open = [&]() -> int {
        if (ctx->timing) SPK_HIP(hipEventRecord(ctx->cc_ev0, st));
        return SPK_OK;
    };
    auto close = [&]() -> int {  // ends the open event pair, synchronises, adds it
        if (ctx->timing) SPK_HIP(hipEventRecord(ctx->cc_ev1, st));
        SPK_HIP(hipStreamSynchronize(st));
        if (ctx->timing) {
            float t = 0.f;
            SPK_HIP(hipEventElapsedTime(&t, ctx->cc_ev0, ctx->cc_ev1));
            ms += (double)t;
        }
        return SPK_OK;
    };
    DevBuf<unsigned int> flags;        // [changed, bad]
    DevBuf<unsigned long long> count;
    SPK_TRY(C.label.alloc((size_t)n_nodes + 1));
    SPK_TRY(flags.alloc(2));
    SPK_TRY(count.alloc(1));
    if (!first) SPK_TRY(open());
    k_cc_init<<<cc_grid(ctx, n_nodes, CC_THREADS), CC_THREADS, 0, st>>>(n_nodes, C.label.p);
    SPK_HIP(hipGetLastError());
    int rounds = 0;
    bool quiet = n_edges == 0;
    const unsigned hook_grid = cc_grid(ctx, n_edges, CC_CHUNK), node_grid = cc_grid(ctx, n_nodes, CC_THREADS);
    while (!quiet) {
        SPK_REQUIRE(rounds < CC_MAX_ROUNDS, SPK_E_LIMIT, "spk_components: no fixed point within 256 rounds");
        if (rounds > 0) SPK_TRY(open());
        SPK_HIP(hipMemsetAsync(flags.p, 0, 2 * sizeof(unsigned int), st));
        if (rounds == 0) k_cc_hook<true><<<hook_grid, CC_THREADS, 0, st>>>(n_nodes, n_edges, eu, ev, C.label.p, flags.p);
        else k_cc_hook<false><<<hook_grid, CC_THREADS, 0, st>>>(n_nodes, n_edges, eu, ev, C.label.p, flags.p);
        SPK_HIP(hipGetLastError());
        k_cc_jump<<<node_grid, CC_THREADS, 0, st>>>(n_nodes, C.label.p, flags.p);
        SPK_HIP(hipGetLastError());
        unsigned int h[2] = {0u, 0u};
        SPK_HIP(hipMemcpyAsync(h, flags.p, sizeof(h), hipMemcpyDeviceToHost, st));
        SPK_TRY(close());
        ++rounds;
        SPK_REQUIRE(h[1] == 0u, bad_code, bad_msg);
        quiet = h[0] == 0u;
    }
    if (rounds > 0) SPK_TRY(open());
    SPK_HIP(hipMemsetAsync(count.p, 0, sizeof(unsigned long long), st));
    k_cc_count<<<node_grid, CC_THREADS, 0, st>>>(n_nodes, C.label.p, count.p);
    SPK_HIP(hipGetLastError());
    unsigned long long n_clusters = 0;
    SPK_HIP(hipMemcpyAsync(&n_clusters, count.p, sizeof(n_clusters), hipMemcpyDeviceToHost, st));
    SPK_TRY(close());
    C.n_nodes = n_nodes;
    C.n_edges = n_edges;
    C.n_clusters = (int64_t)n_clusters;
    C.rounds = rounds;
    C.ms = ctx->timing ? ms : -1.0;
    C.valid = true;
    return SPK_OK;
}

static int cc_events(spk_ctx *ctx) {
    if (!ctx->timing) return SPK_OK;
    if (!ctx->cc_ev0) SPK_HIP(hipEventCreate(&ctx->cc_ev0));
    if (!ctx->cc_ev1) SPK_HIP(hipEventCreate(&ctx->cc_ev1));
    return SPK_OK;
}

}  // namespace spk

using namespace spk;

extern "C" int spk_components(spk_ctx *ctx, int64_t *out_n_nodes, int64_t *out_n_clusters, int *out_rounds) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "spk_components: null ctx");
    SPK_HIP(hipSetDevice(ctx->device));
    ctx->comp.clear();  // whatever happens below, the previous labels are gone
    const Selection &S = ctx->sel;
    SPK_REQUIRE(S.valid, SPK_E_STATE, "spk_components: no selection (run spk_select)");
    SPK_REQUIRE(ctx->codes_valid && S.pairs_epoch == ctx->pairs_epoch && S.gamma_seq == ctx->gamma_seq &&
                    S.fix_seq == ctx->codes_fix_seq,
                SPK_E_STATE, "spk_components: the pairs or codes changed since spk_select");
    SPK_REQUIRE(S.has_rows, SPK_E_STATE, "spk_components: no pair rows (a loaded gamma table)");
    const bool two = ctx->link_type == SPK_LINK_ONLY;
    const Table &t0 = ctx->table[0], &t1 = ctx->table[two ? 1 : 0];
    SPK_REQUIRE(t0.n >= 0 && t1.n >= 0, SPK_E_STATE, "spk_components: no tables");
    const int64_t n_nodes = t0.n + (two ? t1.n : 0), n_edges = S.n;
    SPK_REQUIRE(n_nodes <= (int64_t)UINT32_MAX, SPK_E_LIMIT, "spk_components: more than 2^32 - 1 nodes");
    SPK_TRY(cc_events(ctx));
    Components C;
    DevBuf<uint32_t> eu, ev;
    SPK_TRY(eu.alloc((size_t)n_edges + 1));
    SPK_TRY(ev.alloc((size_t)n_edges + 1));
    if (ctx->timing) SPK_HIP(hipEventRecord(ctx->cc_ev0, ctx->stream));
    if (n_edges > 0) {
        EdgeArgs A{};
        A.n_edges = n_edges;
        A.l = S.l.p;
        A.r = S.r.p;
        A.perm0 = t0.perm.p;
        A.perm1 = t1.perm.p;
        A.n0 = t0.n;
        A.n1 = t1.n;
        A.r_base = two ? (uint32_t)t0.n : 0u;
        A.u = eu.p;
        A.v = ev.p;
        k_cc_edges<<<cc_grid(ctx, n_edges, CC_THREADS), CC_THREADS, 0, ctx->stream>>>(A);
        SPK_HIP(hipGetLastError());
    }
    SPK_TRY(build_components(ctx, n_nodes, n_edges, eu.p, ev.p, SPK_E_STATE,
                             "spk_components: a selected pair names a row outside its table", true, C));
    ctx->comp = std::move(C);
    if (out_n_nodes) *out_n_nodes = ctx->comp.n_nodes;
    if (out_n_clusters) *out_n_clusters = ctx->comp.n_clusters;
    if (out_rounds) *out_rounds = ctx->comp.rounds;
    return SPK_OK;
}

extern "C" int spk_components_edges(spk_ctx *ctx, int64_t n_nodes, int64_t n_edges, const uint32_t *u, const uint32_t *v,
                                    int64_t *out_n_clusters, int *out_rounds) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "spk_components_edges: null ctx");
    SPK_HIP(hipSetDevice(ctx->device));
    ctx->comp.clear();
    SPK_REQUIRE(n_nodes >= 0 && n_edges >= 0, SPK_E_INVALID, "spk_components_edges: negative count");
    SPK_REQUIRE(n_edges == 0 || (u && v), SPK_E_INVALID, "spk_components_edges: null edges");
    SPK_REQUIRE(n_nodes <= (int64_t)UINT32_MAX, SPK_E_LIMIT, "spk_components_edges: more than 2^32 - 1 nodes");
    SPK_TRY(cc_events(ctx));
    Components C;
    DevBuf<uint32_t> eu, ev;
    SPK_TRY(eu.alloc((size_t)n_edges + 1));
    SPK_TRY(ev.alloc((size_t)n_edges + 1));
    if (n_edges > 0) {
        SPK_HIP(hipMemcpyAsync(eu.p, u, (size_t)n_edges * 4, hipMemcpyHostToDevice, ctx->stream));
        SPK_HIP(hipMemcpyAsync(ev.p, v, (size_t)n_edges * 4, hipMemcpyHostToDevice, ctx->stream));
        SPK_HIP(hipStreamSynchronize(ctx->stream));  // u / v are the caller's: done with them on every path below
    }
    SPK_TRY(build_components(ctx, n_nodes, n_edges, eu.p, ev.p, SPK_E_INVALID,
                             "spk_components_edges: a node id is >= n_nodes", false, C));
    ctx->comp = std::move(C);
    if (out_n_clusters) *out_n_clusters = ctx->comp.n_clusters;
    if (out_rounds) *out_rounds = ctx->comp.rounds;
    return SPK_OK;
}

extern "C" int spk_components_copy(spk_ctx *ctx, int64_t start, int64_t count, uint32_t *out_label) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "spk_components_copy: null ctx");
    const Components &C = ctx->comp;
    SPK_REQUIRE(C.valid, SPK_E_STATE, "spk_components_copy: no components (run spk_components)");
    SPK_REQUIRE(start >= 0 && count >= 0 && start + count <= C.n_nodes, SPK_E_INVALID, "spk_components_copy: range");
    SPK_REQUIRE(count == 0 || out_label, SPK_E_INVALID, "spk_components_copy: null out");
    if (!count) return SPK_OK;
    SPK_HIP(hipSetDevice(ctx->device));
    SPK_HIP(hipMemcpyAsync(out_label, C.label.p + start, (size_t)count * 4, hipMemcpyDeviceToHost, ctx->stream));
    SPK_HIP(hipStreamSynchronize(ctx->stream));
    return SPK_OK;
}

extern "C" int spk_components_info(spk_ctx *ctx, int64_t *out_n_nodes, int64_t *out_n_edges, int *out_rounds,
                                   double *out_ms) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "spk_components_info: null ctx");
    const Components &C = ctx->comp;
    if (out_n_nodes) *out_n_nodes = C.valid ? C.n_nodes : -1;
    if (out_n_edges) *out_n_edges = C.valid ? C.n_edges : -1;
    if (out_rounds) *out_rounds = C.valid ? C.rounds : -1;
    if (out_ms) *out_ms = C.valid ? C.ms : -1.0;
    return SPK_OK;
}

extern "C" int spk_components_release(spk_ctx *ctx) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "spk_components_release: null ctx");
    SPK_HIP(hipSetDevice(ctx->device));
    SPK_HIP(hipStreamSynchronize(ctx->stream));
    ctx->comp.clear();
    return SPK_OK;
}
