// Bridges and 2-edge-connected cores of one level of the sweep (gfx950): clusters(t).bridges() on the device.
//
// G is the level's edge multiset over n_nodes nodes: the cumulative range [0, off[level] + cnt[level]) of the sweep's
// edge buffer, padding self-loops (0, 0) included, with the level's labels.  Edge i with u != v is a bridge iff deleting
// that one stored edge leaves u and v in different components; side_u / side_v are the node counts of the two parts its
// cluster falls into; core[v] is the smallest node id of v's component in G minus all bridges.  None of this depends
// on the algorithm, so two runs agree bit for bit although the spanning forest below does not.
//
// Host-driven launches, every one over all the level's edges or over all nodes:
//   k_br_init    depth[v] = 0 at the roots (label[v] == v), "unvisited" elsewhere; parent[v] = v, pedge[v] = -1,
//                mark[v] = 0, sub[v] = 1.
//   k_br_forest  round d, one launch per round: an edge with one end at depth exactly d and the other unvisited claims
//                the other end by a compare-and-swap on its depth word, unvisited -> d + 1, at agent scope; the winner
//                writes parent and pedge (the edge's index in the sweep's buffer, 64-bit) with plain stores.  The host
//                reads a "claimed" word after each round and stops after the first quiet one.
//   k_br_mark    one launch: an edge with u != v that is the tree edge of neither end walks both ends up to their
//                meeting point, the deeper end first, and sets mark[x] on every node x it leaves.
//   k_br_sub     for d = max depth .. 1, one launch each: the nodes at depth d add their subtree count to their
//                parent's (integer atomics).
//   k_br_count / k_br_emit   a node x with depth[x] > 0 and mark[x] == 0 owns the bridge pedge[x]; the bridges are
//                compacted through a cursor (one add per wave), sorted by (u << 32) | v and split into columns.
//   k_br_rest    the edges that are no bridge and no self-loop, compacted the same way; the components' round loop
//                (components_of_edges) over them gives the cores.
//
// Why it is right, for any outcome of the compare-and-swaps:
//   claimed once:    depth[v] leaves "unvisited" only through a successful compare-and-swap, and nothing writes it
//                    after that, so v gets one depth, and one lane -- the winner -- writes parent[v] and pedge[v].
//                    Both words are read only by later launches.
//   depths final     round d extends only from nodes at depth d, whose depth words were written by an earlier launch
//   when read:       (round d - 1, or k_br_init) and never change again; a launch boundary makes them visible to every
//                    CU.  The other end is read with a plain load that may be stale: a stale "unvisited" only makes
//                    the compare-and-swap, which acts on the word itself, fail.  A value other than "unvisited" is never
//                    stale in a harmful way: it is not d (this round writes d + 1 only), so the edge does nothing.
//                    Hence round d claims exactly the unvisited nodes adjacent to depth d: the depths are the BFS
//                    distances from the cluster's smallest id, rounds = max depth + 1, both deterministic; which of
//                    several depth-d neighbours becomes the parent is not.
//   spanning:        the level's labels are the components of exactly these edges, so every node is reached from its
//                    root and the loop ends with no node unvisited.
//   bridges:         a non-tree edge is never a bridge (the tree still connects its ends).  A tree edge (parent[x], x)
//                    is a bridge iff no non-tree edge joins x's subtree to the rest, i.e. iff no fundamental cycle
//                    covers it.  The fundamental cycle of a non-tree edge (a, b) is the two tree paths from a and b to
//                    their meeting point, and the walk marks exactly the nodes whose tree edge lies on them.  A second
//                    copy of a tree edge has another index, so it is a non-tree edge and marks the first: a repeated
//                    edge is no bridge, in either orientation.  A self-loop is skipped everywhere.  This holds for
//                    any spanning tree.
//   marks:           every writer stores 1, the word starts at 0 and is read as data only by later launches.  The load
//                    before the store (a stale 0 costs a store, nothing else) spares a clique's redundant stores of
//                    one word; -DBR_MARK_STORE_ALWAYS leaves it out (the A/B run is a tie: DESIGN.md).
//   sides:           sub[x] after the bottom-up pass is the node count of x's subtree: depth-d nodes are added in
//                    launch d, after all of depth d + 1 were (an earlier launch), and integer adds do not depend on
//                    their order.  Cutting the bridge (parent[x], x) splits the cluster into x's subtree and the rest
//                    -- no other edge leaves the subtree -- so the sides are sub[x] and sub[root] - sub[x].
//   cores:           the components' own argument (spk_components.hip), over the edges that remain.
// Nothing can hang: no workgroup waits for another, there is no spin, no ticket and no cooperative launch; the walk
// is a `for` with the bound 2 * max depth passed from the host (a guard against a state the argument above excludes);
// the forest loop is capped by BR_MAX_ROUNDS and the bottom-up loop by the depth it found.
//
// Cost: the forest reads all of the level's edges once per depth -- the work of a round does not shrink with the
// frontier; the marking costs the sum of the lengths of the fundamental cycles, one lane per non-tree edge; the
// bottom-up pass reads every node once per depth.  Clusters of a linkage are shallow (DESIGN.md has the depths).
//
// Indices: node ids are 32-bit (the sweep's limit, 2^32 - 1 nodes), every edge index and every offset is 64-bit.
// Transient memory, freed at return: 24 bytes per node, 8 per edge for the cores' edge copy, 32 per bridge plus
// rocprim's sort scratch.  Kept: 16 bytes per bridge and 4 per node.
#include <algorithm>

#include "spk_prim.h"

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "spk_bridges.hip targets gfx950 (MI355X) only"
#endif

namespace spk {

constexpr int BR_THREADS = 256;
constexpr int BR_WG_PER_CU = 8;  // capped grid, the workgroups stride over the items (as the components' kernels)
// The forest loop's hard cap: a tree of depth up to BR_MAX_ROUNDS - 1.  A round is a launch and a host round trip
// (tens of microseconds), so the cap bounds a call at a fraction of a second; a deeper tree is a chain of thousands of
// records, not a linkage cluster.  _native.BRIDGES_MAX_ROUNDS mirrors it.
constexpr int BR_MAX_ROUNDS = 4096;
constexpr uint32_t BR_UNVISITED = 0xFFFFFFFFu;

struct BrNodes {
    uint32_t *depth, *parent, *mark, *sub;
    long long *pedge;
};

__global__ __launch_bounds__(BR_THREADS) void k_br_init(int64_t n_nodes, const uint32_t *__restrict__ label, BrNodes N) {
    const int64_t step = (int64_t)gridDim.x * BR_THREADS;
    for (int64_t v = (int64_t)blockIdx.x * BR_THREADS + threadIdx.x; v < n_nodes; v += step) {
        N.depth[v] = (int64_t)label[v] == v ? 0u : BR_UNVISITED;
        N.parent[v] = (uint32_t)v;
        N.pedge[v] = -1ll;
        N.mark[v] = 0u;
        N.sub[v] = 1u;
    }
}

// c, unvisited as far as this lane saw, becomes a child of p at depth d + 1 through edge i -- if this lane is the one
// whose compare-and-swap finds the word still unvisited.
__device__ inline bool br_claim(const BrNodes &N, uint32_t c, uint32_t p, int64_t i, uint32_t d) {
    uint32_t expected = BR_UNVISITED;
    if (!__hip_atomic_compare_exchange_strong(N.depth + (size_t)c, &expected, d + 1u, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_AGENT))
        return false;
    N.parent[(size_t)c] = p;
    N.pedge[(size_t)c] = (long long)i;
    return true;
}

__global__ __launch_bounds__(BR_THREADS) void k_br_forest(int64_t n_edges, const uint32_t *__restrict__ eu,
                                                          const uint32_t *__restrict__ ev, uint32_t d, BrNodes N,
                                                          unsigned int *claimed) {
    bool won = false;
    const int64_t step = (int64_t)gridDim.x * BR_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * BR_THREADS + threadIdx.x; i < n_edges; i += step) {
        const uint32_t u = eu[i], v = ev[i];
        if (u == v) continue;
        const uint32_t du = N.depth[(size_t)u], dv = N.depth[(size_t)v];
        if (du == d && dv == BR_UNVISITED) won |= br_claim(N, v, u, i, d);
        else if (dv == d && du == BR_UNVISITED) won |= br_claim(N, u, v, i, d);
    }
    if (__ballot(won) != 0ull && (threadIdx.x & 63) == 0)
        (void)__hip_atomic_fetch_or(claimed, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ inline void br_set_mark(uint32_t *mark, uint32_t x) {
#ifndef BR_MARK_STORE_ALWAYS  // the A/B variant: tools/build_ab.py OUT.so spk_bridges.hip -DBR_MARK_STORE_ALWAYS
    if (mark[(size_t)x] != 0u) return;
#endif
    mark[(size_t)x] = 1u;
}

// bound = 2 * max depth: the two ends together climb at most depth[u] + depth[v] steps.
__global__ __launch_bounds__(BR_THREADS) void k_br_mark(int64_t n_edges, const uint32_t *__restrict__ eu,
                                                        const uint32_t *__restrict__ ev, BrNodes N, int64_t bound) {
    const int64_t step = (int64_t)gridDim.x * BR_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * BR_THREADS + threadIdx.x; i < n_edges; i += step) {
        uint32_t a = eu[i], b = ev[i];
        if (a == b) continue;
        if (N.pedge[(size_t)a] == (long long)i || N.pedge[(size_t)b] == (long long)i) continue;
        uint32_t da = N.depth[(size_t)a], db = N.depth[(size_t)b];
        for (int64_t s = 0; s < bound; ++s) {
            if (a == b || (da == 0u && db == 0u)) break;  // two roots: excluded by the spanning argument
            if (da >= db) {
                br_set_mark(N.mark, a);
                a = N.parent[(size_t)a];
                --da;
            } else {
                br_set_mark(N.mark, b);
                b = N.parent[(size_t)b];
                --db;
            }
        }
    }
}

__global__ __launch_bounds__(BR_THREADS) void k_br_sub(int64_t n_nodes, uint32_t d, BrNodes N) {
    const int64_t step = (int64_t)gridDim.x * BR_THREADS;
    for (int64_t v = (int64_t)blockIdx.x * BR_THREADS + threadIdx.x; v < n_nodes; v += step)
        if (N.depth[v] == d)
            (void)__hip_atomic_fetch_add(N.sub + (size_t)N.parent[v], N.sub[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// x owns a bridge: it has a tree edge and no cycle covers it
__device__ inline bool br_owns_bridge(const BrNodes &N, int64_t x) {
    const uint32_t d = N.depth[x];
    return d != 0u && d != BR_UNVISITED && N.mark[x] == 0u && N.pedge[x] >= 0;
}

// *count += the nodes that own a bridge (one add per wave)
__global__ __launch_bounds__(BR_THREADS) void k_br_count(int64_t n_nodes, BrNodes N, unsigned long long *count) {
    unsigned long long mine = 0;
    const int64_t step = (int64_t)gridDim.x * BR_THREADS;
    for (int64_t v = (int64_t)blockIdx.x * BR_THREADS + threadIdx.x; v < n_nodes; v += step)
        mine += br_owns_bridge(N, v) ? 1ull : 0ull;
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_down(mine, off, 64);
    if ((threadIdx.x & 63) == 0 && mine)
        (void)__hip_atomic_fetch_add(count, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The place of this lane's item among the wave's kept ones, behind one add of their count to *cursor.  Every lane of the
// wave calls it.  The order of the places varies from run to run; the bridges are sorted afterwards and the cores do
// not depend on the edge order.
__device__ inline unsigned long long br_place(bool keep, unsigned long long *cursor) {
    const unsigned long long m = __ballot(keep);
    if (m == 0ull) return 0ull;
    const int lane = threadIdx.x & 63, leader = __ffsll((long long)m) - 1;
    unsigned long long base = 0ull;
    if (lane == leader)
        base = __hip_atomic_fetch_add(cursor, (unsigned long long)__popcll(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    base = __shfl(base, leader, 64);
    return base + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
}

// key = (u << 32) | v in the stored orientation, val = (side_u << 32) | side_v.  Every place written is below the
// count k_br_count found over the same arrays.
__global__ __launch_bounds__(BR_THREADS) void k_br_emit(int64_t n_nodes, const uint32_t *__restrict__ label,
                                                        const uint32_t *__restrict__ eu, const uint32_t *__restrict__ ev,
                                                        BrNodes N, unsigned long long *cursor, int64_t cap,
                                                        uint64_t *__restrict__ key, uint64_t *__restrict__ val) {
    const int64_t step = (int64_t)gridDim.x * BR_THREADS;
    const int lane = threadIdx.x & 63;
    for (int64_t base = (int64_t)blockIdx.x * BR_THREADS + (threadIdx.x & ~63); base < n_nodes; base += step) {
        const int64_t x = base + lane;
        const bool keep = x < n_nodes && br_owns_bridge(N, x);
        const unsigned long long q = br_place(keep, cursor);
        if (!keep || (int64_t)q >= cap) continue;
        const long long i = N.pedge[x];
        const uint32_t u = eu[i], v = ev[i];
        const uint32_t mine = N.sub[x], rest = N.sub[(size_t)label[x]] - mine;
        const bool child_is_u = (int64_t)u == x;
        key[q] = (uint64_t)u << 32 | (uint64_t)v;
        val[q] = (uint64_t)(child_is_u ? mine : rest) << 32 | (uint64_t)(child_is_u ? rest : mine);
    }
}

__global__ __launch_bounds__(BR_THREADS) void k_br_split(int64_t n, const uint64_t *__restrict__ key,
                                                         const uint64_t *__restrict__ val, uint32_t *__restrict__ u,
                                                         uint32_t *__restrict__ v, uint32_t *__restrict__ su,
                                                         uint32_t *__restrict__ sv) {
    const int64_t step = (int64_t)gridDim.x * BR_THREADS;
    for (int64_t j = (int64_t)blockIdx.x * BR_THREADS + threadIdx.x; j < n; j += step) {
        const uint64_t k = key[j], s = val[j];
        u[j] = (uint32_t)(k >> 32);
        v[j] = (uint32_t)k;
        su[j] = (uint32_t)(s >> 32);
        sv[j] = (uint32_t)s;
    }
}

// The level's edges without the self-loops and the bridges, for the cores' rounds.
__global__ __launch_bounds__(BR_THREADS) void k_br_rest(int64_t n_edges, const uint32_t *__restrict__ eu,
                                                        const uint32_t *__restrict__ ev, BrNodes N,
                                                        unsigned long long *cursor, int64_t cap, uint32_t *__restrict__ ou,
                                                        uint32_t *__restrict__ ov) {
    const int64_t step = (int64_t)gridDim.x * BR_THREADS;
    const int lane = threadIdx.x & 63;
    for (int64_t base = (int64_t)blockIdx.x * BR_THREADS + (threadIdx.x & ~63); base < n_edges; base += step) {
        const int64_t i = base + lane;
        uint32_t u = 0u, v = 0u;
        if (i < n_edges) {
            u = eu[i];
            v = ev[i];
        }
        bool keep = u != v;
        if (keep) {
            const bool bridge = (N.pedge[(size_t)u] == (long long)i && N.mark[(size_t)u] == 0u) ||
                                (N.pedge[(size_t)v] == (long long)i && N.mark[(size_t)v] == 0u);
            keep = !bridge;
        }
        const unsigned long long q = br_place(keep, cursor);
        if (!keep || (int64_t)q >= cap) continue;
        ou[q] = u;
        ov[q] = v;
    }
}

// size[core[v]] += 1.  Consecutive nodes often share a core, so the lanes whose core equals that of the wave's first
// node are counted in the wave and issue one add (as k_cm_nodes).
__global__ __launch_bounds__(BR_THREADS) void k_br_core_sizes(int64_t n_nodes, const uint32_t *__restrict__ core,
                                                              uint32_t *size) {
    const int64_t step = (int64_t)gridDim.x * BR_THREADS;
    const int lane = threadIdx.x & 63;
    for (int64_t base = (int64_t)blockIdx.x * BR_THREADS + (threadIdx.x & ~63); base < n_nodes; base += step) {
        const int64_t v = base + lane;
        const bool valid = v < n_nodes;  // lane 0 always is
        const uint32_t c = valid ? core[v] : 0u;
        const uint32_t c0 = (uint32_t)__shfl((int)c, 0, 64);
        const unsigned long long same = __ballot(valid && c == c0);
        if (lane == 0)
            (void)__hip_atomic_fetch_add(size + (size_t)c0, (uint32_t)__popcll(same), __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_AGENT);
        else if (valid && c != c0)
            (void)__hip_atomic_fetch_add(size + (size_t)c, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// *out = max(*out, size[v]) over every node
__global__ __launch_bounds__(BR_THREADS) void k_br_largest(int64_t n_nodes, const uint32_t *__restrict__ size,
                                                           unsigned long long *out) {
    unsigned long long mine = 0;
    const int64_t step = (int64_t)gridDim.x * BR_THREADS;
    for (int64_t v = (int64_t)blockIdx.x * BR_THREADS + threadIdx.x; v < n_nodes; v += step)
        mine = size[v] > mine ? (unsigned long long)size[v] : mine;
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_down(mine, off, 64);
        mine = o > mine ? o : mine;
    }
    if ((threadIdx.x & 63) == 0 && mine)
        (void)__hip_atomic_fetch_max(out, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

static unsigned br_grid(const spk_ctx *ctx, int64_t items) {
    const int64_t g = (items + BR_THREADS - 1) / BR_THREADS;
    return (unsigned)std::max<int64_t>(std::min<int64_t>(g, BR_WG_PER_CU * (int64_t)ctx->n_cu), 1);
}

// Bridges and cores of `level` of W into B, a local of the caller.  Reads W.label, W.eu, W.ev and the level table.
static int build_bridges(spk_ctx *ctx, const ComponentSweep &W, int level, ClusterBridges &B) {
    hipStream_t st = ctx->stream;
    const int64_t n = W.n_nodes, n_range = W.off[level] + W.cnt[level];
    const uint32_t *lab = W.label.p + (size_t)level * (size_t)n, *eu = W.eu.p, *ev = W.ev.p;
    const unsigned node_grid = br_grid(ctx, n), edge_grid = br_grid(ctx, n_range);
    DevBuf<uint32_t> depth, parent, mark, sub;
    DevBuf<long long> pedge;
    DevBuf<unsigned int> claimed;
    DevBuf<unsigned long long> acc;  // [0] bridges, [1] the bridges' cursor, [2] the rest's cursor, [3] largest core
    SPK_TRY(depth.alloc((size_t)n + 1));
    SPK_TRY(parent.alloc((size_t)n + 1));
    SPK_TRY(mark.alloc((size_t)n + 1));
    SPK_TRY(sub.alloc((size_t)n + 1));
    SPK_TRY(pedge.alloc((size_t)n + 1));
    SPK_TRY(claimed.alloc(1));
    SPK_TRY(acc.alloc(4));
    SPK_TRY(B.core.alloc((size_t)n + 1));
    const BrNodes N{depth.p, parent.p, mark.p, sub.p, pedge.p};
    StageTimer T{ctx};
    // ---- the forest
    SPK_TRY(T.open());
    SPK_HIP(hipMemsetAsync(acc.p, 0, 4 * sizeof(unsigned long long), st));
    k_br_init<<<node_grid, BR_THREADS, 0, st>>>(n, lab, N);
    SPK_HIP(hipGetLastError());
    int rounds = 0;
    for (bool quiet = n_range == 0; !quiet;) {
        SPK_REQUIRE(rounds < BR_MAX_ROUNDS, SPK_E_LIMIT,
                    "spk_cluster_bridges: a cluster's spanning tree is deeper than " + std::to_string(BR_MAX_ROUNDS - 1) +
                        " (tree depth beyond BR_MAX_ROUNDS - 1): a chain of thousands of records");
        SPK_TRY(T.open());
        SPK_HIP(hipMemsetAsync(claimed.p, 0, sizeof(unsigned int), st));
        k_br_forest<<<edge_grid, BR_THREADS, 0, st>>>(n_range, eu, ev, (uint32_t)rounds, N, claimed.p);
        SPK_HIP(hipGetLastError());
        unsigned int h = 0u;
        SPK_HIP(hipMemcpyAsync(&h, claimed.p, sizeof(h), hipMemcpyDeviceToHost, st));
        SPK_TRY(T.close());
        ++rounds;
        quiet = h == 0u;
    }
    const int64_t max_depth = rounds ? rounds - 1 : 0;
    // ---- cycles, subtree counts, the number of bridges
    SPK_TRY(T.open());
    if (max_depth > 0) {
        k_br_mark<<<edge_grid, BR_THREADS, 0, st>>>(n_range, eu, ev, N, 2 * max_depth);
        SPK_HIP(hipGetLastError());
        for (int64_t d = max_depth; d >= 1; --d) {
            k_br_sub<<<node_grid, BR_THREADS, 0, st>>>(n, (uint32_t)d, N);
            SPK_HIP(hipGetLastError());
        }
        k_br_count<<<node_grid, BR_THREADS, 0, st>>>(n, N, acc.p);
        SPK_HIP(hipGetLastError());
    }
    unsigned long long h_bridges = 0ull;
    SPK_HIP(hipMemcpyAsync(&h_bridges, acc.p, sizeof(h_bridges), hipMemcpyDeviceToHost, st));
    SPK_TRY(T.close());
    const int64_t nb = (int64_t)h_bridges;
    SPK_REQUIRE(nb <= n_range, SPK_E_HIP, "spk_cluster_bridges: more bridges than edges");
    // ---- the bridges, sorted, with their sides
    SPK_TRY(B.u.alloc((size_t)nb + 1));
    SPK_TRY(B.v.alloc((size_t)nb + 1));
    SPK_TRY(B.side_u.alloc((size_t)nb + 1));
    SPK_TRY(B.side_v.alloc((size_t)nb + 1));
    const int64_t rest_cap = n_range - nb;
    DevBuf<uint32_t> ru, rv;
    SPK_TRY(ru.alloc((size_t)rest_cap + 4));
    SPK_TRY(rv.alloc((size_t)rest_cap + 4));
    SPK_TRY(T.open());
    if (nb > 0) {
        DevBuf<uint64_t> key, skey, val, sval;
        DevBuf<uint8_t> tmp;
        SPK_TRY(key.alloc((size_t)nb));
        SPK_TRY(skey.alloc((size_t)nb));
        SPK_TRY(val.alloc((size_t)nb));
        SPK_TRY(sval.alloc((size_t)nb));
        k_br_emit<<<node_grid, BR_THREADS, 0, st>>>(n, lab, eu, ev, N, acc.p + 1, nb, key.p, val.p);
        SPK_HIP(hipGetLastError());
        SPK_TRY(sort_pairs_u64(st, tmp, key.p, skey.p, val.p, sval.p, nb));
        k_br_split<<<br_grid(ctx, nb), BR_THREADS, 0, st>>>(nb, skey.p, sval.p, B.u.p, B.v.p, B.side_u.p, B.side_v.p);
        SPK_HIP(hipGetLastError());
        SPK_TRY(T.close());  // the sort's buffers are freed here: done with them
    }
    // ---- the cores: the components' rounds over a compacted copy of the other edges
    unsigned long long h_rest = 0ull;
    if (n_range > 0) {
        SPK_TRY(T.open());
        k_br_rest<<<edge_grid, BR_THREADS, 0, st>>>(n_range, eu, ev, N, acc.p + 2, rest_cap, ru.p, rv.p);
        SPK_HIP(hipGetLastError());
        SPK_HIP(hipMemcpyAsync(&h_rest, acc.p + 2, sizeof(h_rest), hipMemcpyDeviceToHost, st));
        SPK_TRY(T.close());
        SPK_REQUIRE((int64_t)h_rest <= rest_cap, SPK_E_HIP, "spk_cluster_bridges: more edges kept than counted");
    }
    int core_rounds = 0;
    SPK_TRY(components_of_edges(ctx, n, (int64_t)h_rest, ru.p, rv.p, B.core.p, SPK_E_STATE,
                                "spk_cluster_bridges: a node id is >= n_nodes",
                                "spk_cluster_bridges: the cores reached no fixed point within 256 rounds", T, &core_rounds,
                                &B.n_cores));
    // ---- the largest core; sub is free again
    unsigned long long h_largest = 0ull;
    SPK_TRY(T.open());
    if (n > 0) {
        SPK_HIP(hipMemsetAsync(sub.p, 0, (size_t)n * 4, st));
        k_br_core_sizes<<<node_grid, BR_THREADS, 0, st>>>(n, B.core.p, sub.p);
        SPK_HIP(hipGetLastError());
        k_br_largest<<<node_grid, BR_THREADS, 0, st>>>(n, sub.p, acc.p + 3);
        SPK_HIP(hipGetLastError());
    }
    SPK_HIP(hipMemcpyAsync(&h_largest, acc.p + 3, sizeof(h_largest), hipMemcpyDeviceToHost, st));
    SPK_TRY(T.close());
    B.level = level;
    B.n_nodes = n;
    B.n_bridges = nb;
    B.largest_core = (int64_t)h_largest;
    B.depth = max_depth;
    B.rounds = rounds;
    B.ms = T.result();
    return SPK_OK;
}

}  // namespace spk

using namespace spk;

extern "C" int spk_cluster_bridges(spk_ctx *ctx, int level, int64_t *out4) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "spk_cluster_bridges: null ctx");
    ComponentSweep &W = ctx->sweep;
    SPK_REQUIRE(W.valid, SPK_E_STATE, "spk_cluster_bridges: no sweep (run spk_components_sweep)");
    SPK_REQUIRE(level >= 0 && level < W.levels, SPK_E_INVALID, "spk_cluster_bridges: level");
    SPK_REQUIRE(!W.merged, SPK_E_STATE,
                "spk_cluster_bridges: a level of this sweep was merged with other shards' labels, and its stored "
                "edges are one shard's: a bridge of them need not be one of the whole pair set");
    SPK_HIP(hipSetDevice(ctx->device));
    W.bridges.clear();  // whatever happens below, the previous result is gone
    ClusterBridges B;
    SPK_TRY(build_bridges(ctx, W, level, B));
    W.bridges = std::move(B);
    if (out4) {
        out4[0] = W.bridges.n_bridges;
        out4[1] = W.bridges.n_cores;
        out4[2] = W.bridges.largest_core;
        out4[3] = W.bridges.depth;
    }
    return SPK_OK;
}

extern "C" int spk_cluster_bridges_copy(spk_ctx *ctx, int64_t start, int64_t count, uint32_t *out_u, uint32_t *out_v,
                                        uint32_t *out_side_u, uint32_t *out_side_v) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "spk_cluster_bridges_copy: null ctx");
    const ClusterBridges &B = ctx->sweep.bridges;
    SPK_REQUIRE(ctx->sweep.valid && B.level >= 0, SPK_E_STATE,
                "spk_cluster_bridges_copy: no bridges (run spk_cluster_bridges)");
    SPK_REQUIRE(start >= 0 && count >= 0 && start <= B.n_bridges && count <= B.n_bridges - start, SPK_E_INVALID,
                "spk_cluster_bridges_copy: range");
    if (!count) return SPK_OK;
    SPK_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t s = (size_t)start, c = (size_t)count * 4;
    if (out_u) SPK_HIP(hipMemcpyAsync(out_u, B.u.p + s, c, hipMemcpyDeviceToHost, st));
    if (out_v) SPK_HIP(hipMemcpyAsync(out_v, B.v.p + s, c, hipMemcpyDeviceToHost, st));
    if (out_side_u) SPK_HIP(hipMemcpyAsync(out_side_u, B.side_u.p + s, c, hipMemcpyDeviceToHost, st));
    if (out_side_v) SPK_HIP(hipMemcpyAsync(out_side_v, B.side_v.p + s, c, hipMemcpyDeviceToHost, st));
    SPK_HIP(hipStreamSynchronize(st));
    return SPK_OK;
}

extern "C" int spk_cluster_bridges_cores_copy(spk_ctx *ctx, int64_t start, int64_t count, uint32_t *out_core) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "spk_cluster_bridges_cores_copy: null ctx");
    const ClusterBridges &B = ctx->sweep.bridges;
    SPK_REQUIRE(ctx->sweep.valid && B.level >= 0, SPK_E_STATE,
                "spk_cluster_bridges_cores_copy: no bridges (run spk_cluster_bridges)");
    SPK_REQUIRE(start >= 0 && count >= 0 && start <= B.n_nodes && count <= B.n_nodes - start, SPK_E_INVALID,
                "spk_cluster_bridges_cores_copy: range");
    SPK_REQUIRE(count == 0 || out_core, SPK_E_INVALID, "spk_cluster_bridges_cores_copy: null out");
    if (!count) return SPK_OK;
    SPK_HIP(hipSetDevice(ctx->device));
    SPK_HIP(hipMemcpyAsync(out_core, B.core.p + (size_t)start, (size_t)count * 4, hipMemcpyDeviceToHost, ctx->stream));
    SPK_HIP(hipStreamSynchronize(ctx->stream));
    return SPK_OK;
}

extern "C" int spk_cluster_bridges_info(spk_ctx *ctx, int *out_level, int *out_rounds, double *out_ms) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "spk_cluster_bridges_info: null ctx");
    const ClusterBridges &B = ctx->sweep.bridges;
    const bool have = ctx->sweep.valid && B.level >= 0;
    if (out_level) *out_level = have ? B.level : -1;
    if (out_rounds) *out_rounds = have ? B.rounds : -1;
    if (out_ms) *out_ms = have ? B.ms : -1.0;
    return SPK_OK;
}
