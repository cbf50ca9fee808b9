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
//
// Labels at several thresholds (spk_components_sweep*; the reference release has no counterpart, later releases have
// cluster_pairwise_predictions_at_multiple_thresholds and compute_graph_metrics).  With descending thresholds the
// edge sets are nested, so level k's components are unions of level k - 1's.  The edges are given a level each
// (k_sw_level) and bucketed by it (k_sw_scatter), every level's range starting at a multiple of 4 edges -- k_cc_hook
// loads 16 bytes per lane from the start of the range it is given -- and padded with the self-loop (0, 0), which
// cc_hook_edge skips.  Level k then copies level k - 1's final labels into its own array (level 0: k_cc_init) and
// runs the round loop above over an edge set E_k = the edges that are new at level k, plus for every node v the star
// edge (v, label_{k-1}[v]), hooked by the jump launch, which visits every node anyway (k_cc_jump_star).  The argument
// above applies word for word:
//   start state: label_{k-1}[v] is written by a copy in which nothing else touches the word, it is an id of v's
//                level-(k-1) component, which lies inside v's level-k component, and label_{k-1}[v] <= v: invariants
//                (1) and (2) hold at the start as they do after k_cc_init;
//   spanning:    the star edges connect every level-(k-1) component (each node to its smallest id), and the new edges
//                connect those components into level k's, so E_k spans every component of level k;
//   quiet round: it wrote nothing, so every load saw the final array: every edge of E_k joins nodes with one common
//                label, hence all nodes of a level-k component carry one label; every label is a root, a root is <=
//                every node that carries it and is a member, so it is the component's smallest id.
// The other variant (spk_components_sweep_set_mode 1) hooks every edge up to the level with the plain jump; it is
// correct by the same argument with E_k = all edges of level k.  Measured against each other: DESIGN.md.
// A level without new edges runs no round.  The order of the edges inside a level's range depends on the arrival
// order of k_sw_scatter's atomics and varies from run to run; nothing observable depends on it.
//
// The clusters of a multi-GPU job (spk_components_merge, spk_components_sweep_merge).  Every rank labels the graph of
// its shard of the kept pairs, and all ranks number the records the same way, so a rank's final labels are a star
// forest over the common node ids: the edges (v, peer[v]) connect every component of that rank's graph.  The
// components of the union of the shards' pairs are therefore the fixed point of one rank's labels hooked with the
// star edges of every other rank's label array.  It is the round loop above with no hook launch (there is no edge
// list) and the node launch k_cc_jump_stars, which does k_cc_jump's jump and then, for each peer p, hooks
// (v, peer_p[v]).  The argument carries over:
//   start state: the rank's own final labels were written by launches that have completed: invariants (1) and (2)
//                hold (for the union's components, which contain the rank's own), and label[v] <= v;
//   spanning:    the forest in `label` spans the rank's own components when the merge starts, and here nothing else
//                does -- the rank's edge list is gone, where the rounds above hook every edge again and so repair a
//                link that a hook of a non-root (a climb cut short, a stale load) has cut.  So the merge's hook
//                (cc_hook_root) re-parents the larger end only by a compare-and-swap against its own id: only a root
//                gains a parent, the jump moves a node to a former ancestor, trees only ever merge, and the forest
//                keeps spanning the rank's components; the star arrays span every peer's components; together they
//                span every component of the union.  (Lowering a non-root here lost about one merge in 2,000 on the
//                65,536-node path: the rank's own forest came out split.)
//   quiet round: it wrote nothing, so every load saw the final array: every star edge of every peer joins nodes
//                with one common label, hence (with the forest) all nodes of a component of the union carry one
//                label; every label is a root, a root is <= every node that carries it and is a member, so it is the
//                component's smallest id;
//   progress:    no workgroup waits for another, every loop in the kernel is bounded (CC_PEER_BATCH, n_peers, CC_CLIMB)
//                and CC_MAX_ROUNDS caps the host loop.
// A peer array comes from outside (another process, the host): the first round validates every entry before anything
// is indexed with it -- q <= v, and so q < n_nodes -- and reports through flags[1], as the first hook launch does for
// an edge list.  (2) needs nothing more of a peer array than that: any array with peer[v] <= v names some graph, and
// the result is the components of the union with that graph.  The peer rows are read once per round and streamed past
// the caches (non-temporal loads), so the labels, which every climb reads, keep them.
#include <algorithm>

#include "spk_internal.h"

namespace spk {

constexpr int CC_THREADS = 256;
constexpr int CC_VEC = 4;                                 // edges per lane and chunk: one 16-byte load of u, one of v
constexpr int64_t CC_CHUNK = (int64_t)CC_THREADS * CC_VEC;  // edges per workgroup step; _native.COMPONENTS_CHUNK mirrors it
constexpr int CC_WG_PER_CU = 8;                           // capped grid, the workgroups stride over the chunks (as k_select)
constexpr int CC_CLIMB = 8;                               // loads of one climb; tools/emulate_components.py mirrors it
constexpr int CC_MAX_ROUNDS = 256;                        // the loop's hard cap (SPK_E_LIMIT beyond it)
constexpr int CC_MAX_PEERS = SPK_COMPONENTS_MAX_PEERS;    // label arrays of one merge; _native.COMPONENTS_MAX_PEERS mirrors it
constexpr int CC_PEER_BATCH = 4;                          // peer entries a lane loads before it hooks them

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

// ---- the sweep: labels at several thresholds ------------------------------------------------------------------------
constexpr int SW_BUCKETS = SPK_SWEEP_MAX_LEVELS + 1;  // the levels, and "in no level"

// lev[i] = the first level whose threshold edge i's score exceeds (the thresholds descend, so the edge is in every
// later level too), L for an edge of no level (a NaN, or a score <= every threshold); hist[b] += the edges of bucket b.
// The score is mpat[code[i]] (a selection's match_probability), score[i], or absent (L = 1, every edge in level 0).
__global__ __launch_bounds__(CC_THREADS) void k_sw_level(int64_t n_edges, const uint32_t *__restrict__ code,
                                                         const double *__restrict__ mpat,
                                                         const double *__restrict__ score, int L,
                                                         const double *__restrict__ thr, uint8_t *__restrict__ lev,
                                                         unsigned long long *hist) {
    __shared__ unsigned long long s_cnt[SW_BUCKETS];
    if (threadIdx.x < SW_BUCKETS) s_cnt[threadIdx.x] = 0ull;
    __syncthreads();
    const int64_t step = (int64_t)gridDim.x * CC_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x; i < n_edges; i += step) {
        int b = 0;
        if (mpat || score) {
            // code[i] < n_patterns without a guard here: spk_select* keeps only pairs whose code its pattern pass
            // checked, and spk_select_best copies those codes (k_select_decode reads mpat the same way)
            const double s = mpat ? mpat[code[i]] : score[i];
            b = L;
            for (int k = L - 1; k >= 0; --k)
                if (s > thr[k]) b = k;
        }
        lev[i] = (uint8_t)b;
        (void)atomicAdd(&s_cnt[b], 1ull);
    }
    __syncthreads();
    if (threadIdx.x < SW_BUCKETS && s_cnt[threadIdx.x])
        (void)__hip_atomic_fetch_add(hist + threadIdx.x, s_cnt[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Edge i goes to the next free place of its level's range: cursor[b] starts at the range's first place, a workgroup
// takes the places of its 256 edges with one add per level, and the edges rank themselves inside that in LDS.  The
// order inside a range therefore varies from run to run; nothing observable depends on it (labels and metrics are
// functions of the edge multiset).  An edge of no level is dropped.  Every place written lies in [off[b], off[b] +
// cnt[b]): the counts come from the same lev array.
__global__ __launch_bounds__(CC_THREADS) void k_sw_scatter(int64_t n_edges, int L, const uint8_t *__restrict__ lev,
                                                           const uint32_t *__restrict__ u, const uint32_t *__restrict__ v,
                                                           unsigned long long *cursor, uint32_t *__restrict__ ou,
                                                           uint32_t *__restrict__ ov) {
    __shared__ unsigned int s_cnt[SW_BUCKETS];
    __shared__ unsigned long long s_base[SW_BUCKETS];
    const int64_t n_chunks = (n_edges + CC_THREADS - 1) / CC_THREADS;
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const int64_t i = c * CC_THREADS + threadIdx.x;
        const int b = i < n_edges ? (int)lev[i] : L;
        if (threadIdx.x < SW_BUCKETS) s_cnt[threadIdx.x] = 0u;
        __syncthreads();
        const unsigned int rank = b < L ? atomicAdd(&s_cnt[b], 1u) : 0u;
        __syncthreads();
        if ((int)threadIdx.x < L && s_cnt[threadIdx.x])
            s_base[threadIdx.x] = __hip_atomic_fetch_add(cursor + threadIdx.x, (unsigned long long)s_cnt[threadIdx.x],
                                                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        if (b < L) {
            const size_t q = (size_t)(s_base[b] + rank);
            ou[q] = u[i];
            ov[q] = v[i];
        }
        __syncthreads();  // s_cnt and s_base are rewritten by the next chunk
    }
}

// k_cc_jump of a level k > 0, which also hooks, for every node v, the star edge (v, prev[v]), prev = the final labels
// of level k - 1 (read only here).
__global__ __launch_bounds__(CC_THREADS) void k_cc_jump_star(int64_t n_nodes, uint32_t *label,
                                                             const uint32_t *__restrict__ prev, unsigned int *flags) {
    bool changed = false, bad = false;
    const int64_t step = (int64_t)gridDim.x * CC_THREADS;
    for (int64_t v = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x; v < n_nodes; v += step) {
        const uint32_t p = label[v];
        if ((int64_t)p != v) {
            const uint32_t r = cc_climb(label, p);
            if (r < p) {
                changed = true;
                (void)__hip_atomic_fetch_min(label + v, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        cc_hook_edge<false>(label, n_nodes, (uint32_t)v, prev[v], changed, bad);
    }
    cc_raise(flags, changed, false);
}

// Star arrays hooked by the node launch: row p is rows + p * stride, [n_nodes] entries read.  `foreign`: the rows come
// from outside this library's own launches (a merge's peers) and the first round validates them; otherwise one row, the
// previous level's labels of a sweep.
struct Stars {
    const uint32_t *rows = nullptr;
    int n = 0;
    int64_t stride = 0;
    bool foreign = false;
};

// cc_hook_edge of a merge.  There the rank's own components live in `label` alone (its edge list is gone), so a hook
// must never cut a node off its parent: the larger end is re-parented only while it is a root, by a compare-and-swap
// against its own id, which acts on the word itself and not on a possibly stale load.  A climb that stopped short of
// the root (CC_CLIMB loads) or over stale labels then fails its swap, reports the round as not quiet and is taken up
// again in the next one, after the jumps have shortened the chains.  With that, parents change only by a root gaining
// one (two trees merge) and by a jump to a former ancestor (which is still in the node's tree): trees never split.
__device__ inline void cc_hook_root(uint32_t *label, uint32_t u, uint32_t v, bool &changed) {
    if (u == v) return;
    uint32_t a = cc_load(label, u), b = cc_load(label, v);
    if (a == b) return;
    a = cc_climb(label, a);
    b = cc_climb(label, b);
    if (a == b) return;  // one tree, not flat yet: the jump lowers a label in it and reports that
    changed = true;
    uint32_t hi = a > b ? a : b;
    const uint32_t lo = a > b ? b : a;
    (void)__hip_atomic_compare_exchange_strong(label + (size_t)hi, &hi, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT);
}

// k_cc_jump of a merge, which also hooks, for every node v and every peer p, the star edge (v, peer_p[v]).  An entry
// equal to v (a record that is a cluster of its own on that rank: most are) costs its own load and nothing else.  A
// lane's CC_PEER_BATCH loads are issued together; a row starts at any 4-byte alignment (stride is the caller's), so the
// loads are scalar, coalesced over the wave's consecutive v.  CHECK: the first round, which validates every entry
// before it indexes the labels with it: q <= v, and so q < n_nodes.
template <bool CHECK>
__global__ __launch_bounds__(CC_THREADS) void k_cc_jump_stars(int64_t n_nodes, uint32_t *label,
                                                              const uint32_t *__restrict__ peer, int n_peers,
                                                              int64_t stride, unsigned int *flags) {
    bool changed = false, bad = false;
    const int64_t step = (int64_t)gridDim.x * CC_THREADS;
    for (int64_t v = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x; v < n_nodes; v += step) {
        const uint32_t p = label[v];
        if ((int64_t)p != v) {
            const uint32_t r = cc_climb(label, p);
            if (r < p) {
                changed = true;
                (void)__hip_atomic_fetch_min(label + v, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        for (int p0 = 0; p0 < n_peers; p0 += CC_PEER_BATCH) {
            uint32_t q[CC_PEER_BATCH];
#pragma unroll
            for (int j = 0; j < CC_PEER_BATCH; ++j)  // past the last peer: v itself, which is skipped
                q[j] = p0 + j < n_peers ? __builtin_nontemporal_load(peer + ((int64_t)(p0 + j) * stride + v)) : (uint32_t)v;
#pragma unroll
            for (int j = 0; j < CC_PEER_BATCH; ++j) {
                if ((int64_t)q[j] == v) continue;
                if (CHECK && ((int64_t)q[j] > v || (int64_t)q[j] >= n_nodes)) {
                    bad = true;
                    continue;
                }
                cc_hook_root(label, (uint32_t)v, q[j], changed);
            }
        }
    }
    cc_raise(flags, changed, bad);
}

// ---- metrics of one level ------------------------------------------------------------------------------------------
// degree[x] += 1 for one end x per active lane.  AGG: the lanes whose end equals that of the wave's first active lane
// issue one add of their count (the lowest of them does); the others add on their own.
template <bool AGG>
__device__ inline void cm_degree_add(uint32_t *degree, uint32_t x) {
    if (AGG) {
        const uint32_t x0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)x);
        const unsigned long long same = __ballot(x == x0);
        if (x == x0) {
            if ((int)(threadIdx.x & 63) == __ffsll((long long)same) - 1)
                (void)__hip_atomic_fetch_add(degree + (size_t)x0, (uint32_t)__popcll(same), __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
    }
    (void)__hip_atomic_fetch_add(degree + (size_t)x, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Two adds per edge.  AGG (the default; spk_cluster_metrics_set_mode 0 turns it off) counts the lanes that share the
// first lane's end inside the wave before the add: 0.27 -> 0.18 ms for the whole call on the hub graph, 11.6 -> 0.41 ms
// on one star of 10^6 leaves, no difference on the random graph.
template <bool AGG>
__global__ __launch_bounds__(CC_THREADS) void k_cm_degree(int64_t n_edges, const uint32_t *__restrict__ eu,
                                                          const uint32_t *__restrict__ ev, uint32_t *degree) {
    const int64_t step = (int64_t)gridDim.x * CC_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x; i < n_edges; i += step) {
        cm_degree_add<AGG>(degree, eu[i]);
        cm_degree_add<AGG>(degree, ev[i]);
    }
}

// Per node v: size[label[v]] += 1, degree_sum[label[v]] += degree[v], max_degree[label[v]] = max(., degree[v]).
// Consecutive nodes often share a label (one cluster of 10^6 records would put 3 x 10^6 atomics on three words), so
// the lanes whose label equals that of the wave's first node are reduced in the wave and their leader issues the three
// atomics; the other lanes issue their own.  Every trip of the loop is taken by the whole wave (the shuffles need it).
__global__ __launch_bounds__(CC_THREADS) void k_cm_nodes(int64_t n_nodes, const uint32_t *__restrict__ label,
                                                         const uint32_t *__restrict__ degree, uint32_t *size,
                                                         unsigned long long *degree_sum, uint32_t *max_degree) {
    const int64_t step = (int64_t)gridDim.x * CC_THREADS;
    const int lane = threadIdx.x & 63;
    for (int64_t base = (int64_t)blockIdx.x * CC_THREADS + (threadIdx.x & ~63); base < n_nodes; base += step) {
        const int64_t v = base + lane;
        const bool valid = v < n_nodes;  // lane 0 always is
        const uint32_t l = valid ? label[v] : 0u, d = valid ? degree[v] : 0u;
        const uint32_t l0 = (uint32_t)__shfl((int)l, 0, 64);
        const bool with_first = valid && l == l0;
        unsigned int cnt = with_first ? 1u : 0u, mx = with_first ? d : 0u;
        unsigned long long sum = with_first ? (unsigned long long)d : 0ull;
        for (int off = 32; off > 0; off >>= 1) {
            cnt += __shfl_down(cnt, off, 64);
            sum += __shfl_down(sum, off, 64);
            const unsigned int o = __shfl_down(mx, off, 64);
            mx = o > mx ? o : mx;
        }
        if (lane == 0) {
            (void)__hip_atomic_fetch_add(size + (size_t)l0, cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (sum) (void)__hip_atomic_fetch_add(degree_sum + (size_t)l0, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (mx) (void)__hip_atomic_fetch_max(max_degree + (size_t)l0, mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else if (valid && !with_first) {
            (void)__hip_atomic_fetch_add(size + (size_t)l, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (d) {
                (void)__hip_atomic_fetch_add(degree_sum + (size_t)l, (unsigned long long)d, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT);
                (void)__hip_atomic_fetch_max(max_degree + (size_t)l, d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

// out[0] += the roots with size >= 2, out[1] += their sizes, out[2] = max(out[2], size) over every root
__global__ __launch_bounds__(CC_THREADS) void k_cm_scalars(int64_t n_nodes, const uint32_t *__restrict__ label,
                                                           const uint32_t *__restrict__ size, unsigned long long *out) {
    unsigned long long multi = 0, nodes = 0, largest = 0;
    const int64_t step = (int64_t)gridDim.x * CC_THREADS;
    for (int64_t v = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x; v < n_nodes; v += step) {
        if ((int64_t)label[v] != v) continue;
        const unsigned long long s = size[v];
        largest = s > largest ? s : largest;
        if (s >= 2) {
            ++multi;
            nodes += s;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        multi += __shfl_down(multi, off, 64);
        nodes += __shfl_down(nodes, off, 64);
        const unsigned long long o = __shfl_down(largest, off, 64);
        largest = o > largest ? o : largest;
    }
    if ((threadIdx.x & 63) == 0 && largest) {
        if (multi) (void)__hip_atomic_fetch_add(out, multi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (nodes) (void)__hip_atomic_fetch_add(out + 1, nodes, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        (void)__hip_atomic_fetch_max(out + 2, largest, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- the round loop ---------------------------------------------------------------------------------------------------
// Brings lab [n_nodes] to its fixed point and counts its clusters.  lab holds a start state for which invariants (1) and
// (2) hold (k_cc_init, a copy of the previous level's labels, or a finished result about to be merged).  The rounds
// hook the edges (hu, hv) [hn] and the star edges of S; the hook launch is left out when hn = 0, and without edges and
// without star arrays no round runs.  flags [2] and count [1] are the caller's device scratch.
// T may be open around the caller's own launches (the edge build, the start state): they count into round 0's interval.
static int cc_fixed_point(spk_ctx *ctx, int64_t n_nodes, const uint32_t *hu, const uint32_t *hv, int64_t hn,
                          uint32_t *lab, const Stars &S, unsigned int *flags, unsigned long long *count,
                          int bad_code, const char *bad_msg, const char *limit_msg, StageTimer &T, int *out_rounds,
                          int64_t *out_n_clusters) {
    hipStream_t st = ctx->stream;
    const unsigned hook_grid = cc_grid(ctx, hn, CC_CHUNK), node_grid = cc_grid(ctx, n_nodes, CC_THREADS);
    int rounds = 0;
    bool quiet = hn == 0 && S.n == 0;
    while (!quiet) {
        SPK_REQUIRE(rounds < CC_MAX_ROUNDS, SPK_E_LIMIT, limit_msg);
        SPK_TRY(T.open());
        SPK_HIP(hipMemsetAsync(flags, 0, 2 * sizeof(unsigned int), st));
        if (hn > 0) {
            if (rounds == 0) k_cc_hook<true><<<hook_grid, CC_THREADS, 0, st>>>(n_nodes, hn, hu, hv, lab, flags);
            else k_cc_hook<false><<<hook_grid, CC_THREADS, 0, st>>>(n_nodes, hn, hu, hv, lab, flags);
            SPK_HIP(hipGetLastError());
        }
        if (S.foreign && rounds == 0)
            k_cc_jump_stars<true><<<node_grid, CC_THREADS, 0, st>>>(n_nodes, lab, S.rows, S.n, S.stride, flags);
        else if (S.foreign)
            k_cc_jump_stars<false><<<node_grid, CC_THREADS, 0, st>>>(n_nodes, lab, S.rows, S.n, S.stride, flags);
        else if (S.n) k_cc_jump_star<<<node_grid, CC_THREADS, 0, st>>>(n_nodes, lab, S.rows, flags);
        else k_cc_jump<<<node_grid, CC_THREADS, 0, st>>>(n_nodes, lab, flags);
        SPK_HIP(hipGetLastError());
        unsigned int h[2] = {0u, 0u};  // [changed, bad]
        SPK_HIP(hipMemcpyAsync(h, flags, sizeof(h), hipMemcpyDeviceToHost, st));
        SPK_TRY(T.close());
        ++rounds;
        SPK_REQUIRE(h[1] == 0u, bad_code, bad_msg);
        quiet = h[0] == 0u;
    }
    SPK_TRY(T.open());
    SPK_HIP(hipMemsetAsync(count, 0, sizeof(unsigned long long), st));
    k_cc_count<<<node_grid, CC_THREADS, 0, st>>>(n_nodes, lab, count);
    SPK_HIP(hipGetLastError());
    unsigned long long n_clusters = 0;
    SPK_HIP(hipMemcpyAsync(&n_clusters, count, sizeof(n_clusters), hipMemcpyDeviceToHost, st));
    SPK_TRY(T.close());
    *out_rounds = rounds;
    *out_n_clusters = (int64_t)n_clusters;
    return SPK_OK;
}

// k_cc_init and the round loop over one edge list (spk_internal.h): spk_components*, and the cores of spk_bridges.hip.
int components_of_edges(spk_ctx *ctx, int64_t n_nodes, int64_t n_edges, const uint32_t *eu, const uint32_t *ev,
                        uint32_t *label, int bad_code, const char *bad_msg, const char *limit_msg, StageTimer &T,
                        int *out_rounds, int64_t *out_n_clusters) {
    DevBuf<unsigned int> flags;
    DevBuf<unsigned long long> count;
    SPK_TRY(flags.alloc(2));
    SPK_TRY(count.alloc(1));
    SPK_TRY(T.open());
    k_cc_init<<<cc_grid(ctx, n_nodes, CC_THREADS), CC_THREADS, 0, ctx->stream>>>(n_nodes, label);
    SPK_HIP(hipGetLastError());
    return cc_fixed_point(ctx, n_nodes, eu, ev, n_edges, label, Stars{}, flags.p, count.p, bad_code, bad_msg, limit_msg,
                          T, out_rounds, out_n_clusters);
}

// Labels of the graph (eu, ev) [n_edges] over n_nodes nodes into C, a local of the caller.  T: possibly open around
// the caller's edge build.
static int build_components(spk_ctx *ctx, int64_t n_nodes, int64_t n_edges, const uint32_t *eu, const uint32_t *ev,
                            int bad_code, const char *bad_msg, StageTimer &T, Components &C) {
    SPK_TRY(C.label.alloc((size_t)n_nodes + 1));
    SPK_TRY(components_of_edges(ctx, n_nodes, n_edges, eu, ev, C.label.p, bad_code, bad_msg,
                                "spk_components: no fixed point within 256 rounds", T, &C.rounds, &C.n_clusters));
    C.n_nodes = n_nodes;
    C.n_edges = n_edges;
    C.ms = T.result();
    C.valid = true;
    return SPK_OK;
}

// The current selection's pairs as edges (eu, ev) [ctx->sel.n] over *n_nodes node ids, for spk_components and
// spk_components_sweep (`who`): the state checks, then k_cc_edges inside an interval of T that it leaves open.
// field: the score the caller goes on to read, SPK_SEL_ALL for none.
static int selection_edges(spk_ctx *ctx, const char *who, int field, StageTimer &T, DevBuf<uint32_t> &eu,
                           DevBuf<uint32_t> &ev, int64_t *n_nodes) {
    const std::string w(who);
    const Selection &S = ctx->sel;
    SPK_REQUIRE(S.valid, SPK_E_STATE, w + ": no selection (run spk_select)");
    SPK_REQUIRE(S.current(ctx), SPK_E_STATE, w + ": the pairs or codes changed since spk_select");
    SPK_REQUIRE(S.has_rows, SPK_E_STATE, w + ": no pair rows (a loaded gamma table)");
    SPK_REQUIRE(field != SPK_SEL_MP || S.has_mp, SPK_E_STATE, w + ": spk_select got no m / u");
    SPK_REQUIRE(field != SPK_SEL_TF_MP || S.has_tf, SPK_E_STATE,
                w + ": the selection was made without tf tables (spk_select)");
    const NodeSpace N = node_space(ctx);
    SPK_REQUIRE(N.n0 >= 0 && N.n1 >= 0, SPK_E_STATE, w + ": no tables");
    SPK_REQUIRE(N.n_nodes <= (int64_t)UINT32_MAX, SPK_E_LIMIT, w + ": more than 2^32 - 1 nodes");
    *n_nodes = N.n_nodes;
    SPK_TRY(eu.alloc((size_t)S.n + 1));
    SPK_TRY(ev.alloc((size_t)S.n + 1));
    if (S.n == 0) return SPK_OK;
    SPK_TRY(T.open());
    EdgeArgs A{};
    A.n_edges = S.n;
    A.l = S.l.p;
    A.r = S.r.p;
    A.perm0 = N.t0->perm.p;
    A.perm1 = N.t1->perm.p;
    A.n0 = N.n0;
    A.n1 = N.n1;
    A.r_base = (uint32_t)N.r_base;
    A.u = eu.p;
    A.v = ev.p;
    k_cc_edges<<<cc_grid(ctx, S.n, CC_THREADS), CC_THREADS, 0, ctx->stream>>>(A);
    SPK_HIP(hipGetLastError());
    return SPK_OK;
}

// L and the thresholds of a sweep call; `all`: the call has no scores (SPK_SEL_ALL, or host edges without thresholds)
static int sweep_thresholds(const char *who, bool all, int n_thresholds, const double *thresholds, int *out_levels) {
    const std::string w(who);
    if (all) {
        SPK_REQUIRE(n_thresholds == 0, SPK_E_INVALID, w + ": SPK_SEL_ALL takes no thresholds");
        *out_levels = 1;
        return SPK_OK;
    }
    SPK_REQUIRE(n_thresholds >= 1 && n_thresholds <= SPK_SWEEP_MAX_LEVELS, SPK_E_INVALID, w + ": 1 to 32 thresholds");
    SPK_REQUIRE(thresholds, SPK_E_INVALID, w + ": null thresholds");
    for (int k = 0; k < n_thresholds; ++k) {
        SPK_REQUIRE(thresholds[k] == thresholds[k], SPK_E_INVALID, w + ": a threshold is NaN");
        SPK_REQUIRE(k == 0 || thresholds[k] < thresholds[k - 1], SPK_E_INVALID,
                    w + ": the thresholds must be strictly descending");
    }
    *out_levels = n_thresholds;
    return SPK_OK;
}

// The sweep of the graph (eu0, ev0) [n_raw] over n_nodes nodes into S, a local of the caller.  The edges' scores are
// mpat[code[i]], score[i], or absent (L = 1; thresholds is not read then).  T: possibly open around the caller's edge
// build.
static int build_sweep(spk_ctx *ctx, int64_t n_nodes, int64_t n_raw, const uint32_t *eu0, const uint32_t *ev0,
                       const uint32_t *code, const double *mpat, const double *score, int L, const double *thresholds,
                       int bad_code, const char *bad_msg, StageTimer &T, ComponentSweep &S) {
    hipStream_t st = ctx->stream;
    DevBuf<uint8_t> lev;
    DevBuf<unsigned long long> hist;  // [SW_BUCKETS] counts | [SW_BUCKETS] cursors | 1 cluster count
    DevBuf<double> thr;
    DevBuf<unsigned int> flags;       // [changed, bad]
    SPK_TRY(lev.alloc((size_t)n_raw + 1));
    SPK_TRY(hist.alloc(2 * SW_BUCKETS + 1));
    SPK_TRY(thr.alloc(SPK_SWEEP_MAX_LEVELS));
    SPK_TRY(flags.alloc(2));
    unsigned long long *cursor = hist.p + SW_BUCKETS, *count = hist.p + 2 * SW_BUCKETS;
    const unsigned raw_grid = cc_grid(ctx, n_raw, CC_THREADS), node_grid = cc_grid(ctx, n_nodes, CC_THREADS);
    // ---- a level per edge, the levels' counts, their padded ranges
    unsigned long long h[SW_BUCKETS] = {};
    if (n_raw > 0) {
        SPK_TRY(T.open());
        if (mpat || score) SPK_HIP(hipMemcpyAsync(thr.p, thresholds, (size_t)L * 8, hipMemcpyHostToDevice, st));
        SPK_HIP(hipMemsetAsync(hist.p, 0, SW_BUCKETS * sizeof(unsigned long long), st));
        k_sw_level<<<raw_grid, CC_THREADS, 0, st>>>(n_raw, code, mpat, score, L, thr.p, lev.p, hist.p);
        SPK_HIP(hipGetLastError());
        SPK_HIP(hipMemcpyAsync(h, hist.p, sizeof(h), hipMemcpyDeviceToHost, st));
    }
    SPK_TRY(T.close());  // the thresholds are the caller's: done with them
    S.levels = L;
    S.n_nodes = n_nodes;
    S.off.assign(L + 1, 0);
    S.cnt.assign(L, 0);
    S.n_edges.assign(L, 0);
    S.n_clusters.assign(L, 0);
    S.rounds.assign(L, 0);
    unsigned long long start[SW_BUCKETS] = {};
    for (int k = 0; k < L; ++k) {
        S.cnt[k] = (int64_t)h[k];
        S.n_edges[k] = (k ? S.n_edges[k - 1] : 0) + S.cnt[k];
        S.off[k + 1] = (S.off[k] + S.cnt[k] + CC_VEC - 1) / CC_VEC * CC_VEC;  // k_cc_hook's 16-byte loads start here
        start[k] = (unsigned long long)S.off[k];
    }
    const int64_t n_kept = S.n_edges[L - 1], padded = S.off[L];
    SPK_TRY(S.eu.alloc((size_t)padded + CC_VEC));
    SPK_TRY(S.ev.alloc((size_t)padded + CC_VEC));
    SPK_TRY(S.label.alloc((size_t)L * (size_t)n_nodes + 1));
    if (n_kept > 0) {
        SPK_TRY(T.open());
        // the padding is the self-loop (0, 0), which cc_hook_edge skips (n_kept > 0 with n_nodes = 0 fails its check)
        SPK_HIP(hipMemsetAsync(S.eu.p, 0, (size_t)padded * 4, st));
        SPK_HIP(hipMemsetAsync(S.ev.p, 0, (size_t)padded * 4, st));
        SPK_HIP(hipMemcpyAsync(cursor, start, sizeof(start), hipMemcpyHostToDevice, st));
        k_sw_scatter<<<raw_grid, CC_THREADS, 0, st>>>(n_raw, L, lev.p, eu0, ev0, cursor, S.eu.p, S.ev.p);
        SPK_HIP(hipGetLastError());
        SPK_TRY(T.close());  // `start` is a local: done with it
    }
    // ---- level after level
    const bool prefix = ctx->sweep_mode == 1;
    for (int k = 0; k < L; ++k) {
        uint32_t *lab = S.label.p + (size_t)k * (size_t)n_nodes;
        const uint32_t *prev = k ? lab - (size_t)n_nodes : nullptr;
        // no new edge: no round, the previous level's labels are this level's
        const int64_t hn = !S.cnt[k] ? 0 : prefix ? S.off[k] + S.cnt[k] : S.cnt[k];
        const uint32_t *hu = S.eu.p + (prefix ? 0 : S.off[k]), *hv = S.ev.p + (prefix ? 0 : S.off[k]);
        SPK_TRY(T.open());
        if (!prev) {
            k_cc_init<<<node_grid, CC_THREADS, 0, st>>>(n_nodes, lab);
            SPK_HIP(hipGetLastError());
        } else if (n_nodes > 0) {
            SPK_HIP(hipMemcpyAsync(lab, prev, (size_t)n_nodes * 4, hipMemcpyDeviceToDevice, st));
        }
        Stars stars;  // the previous level's labels, for a level that has new edges to hook
        if (prev && !prefix && hn > 0) {
            stars.rows = prev;
            stars.n = 1;
            stars.stride = n_nodes;
        }
        SPK_TRY(cc_fixed_point(ctx, n_nodes, hu, hv, hn, lab, stars, flags.p, count, bad_code, bad_msg,
                               "spk_components_sweep: no fixed point within 256 rounds", T, &S.rounds[k],
                               &S.n_clusters[k]));
    }
    S.ms = T.result();
    S.valid = true;
    return SPK_OK;
}

static void sweep_outputs(const ComponentSweep &S, int64_t *out_n_edges, int64_t *out_n_clusters, int *out_rounds) {
    for (int k = 0; k < S.levels; ++k) {
        if (out_n_edges) out_n_edges[k] = S.n_edges[k];
        if (out_n_clusters) out_n_clusters[k] = S.n_clusters[k];
        if (out_rounds) out_rounds[k] = S.rounds[k];
    }
}

// The argument checks spk_components_merge and spk_components_sweep_merge (`who`) share; nothing is touched before them.
static int merge_arguments(const char *who, int n_peers, const uint32_t *peer_labels, int64_t stride, int64_t n_nodes) {
    const std::string w(who);
    SPK_REQUIRE(n_peers >= 1 && n_peers <= CC_MAX_PEERS, SPK_E_INVALID, w + ": 1 to 64 peers");
    SPK_REQUIRE(peer_labels, SPK_E_INVALID, w + ": null peer_labels");
    SPK_REQUIRE(stride >= n_nodes, SPK_E_INVALID, w + ": stride < n_nodes");
    SPK_REQUIRE(stride <= (int64_t)UINT32_MAX, SPK_E_INVALID, w + ": stride beyond 2^32 - 1");
    return SPK_OK;
}

// lab [n_nodes], a finished result, to the fixed point of itself hooked with the peers' star edges.  A host pointer is
// uploaded into a buffer of this call.  Whatever fails here may have lowered labels already: the caller drops the result.
static int merge_labels(spk_ctx *ctx, const char *who, int64_t n_nodes, uint32_t *lab, int n_peers,
                        const uint32_t *peer_labels, int64_t stride, int on_device, StageTimer &T, int *out_rounds,
                        int64_t *out_n_clusters) {
    const std::string w(who);
    DevBuf<uint32_t> up;
    DevBuf<unsigned int> flags;
    DevBuf<unsigned long long> count;
    SPK_TRY(flags.alloc(2));
    SPK_TRY(count.alloc(1));
    Stars S;
    S.rows = peer_labels;
    S.n = n_peers;
    S.stride = stride;
    S.foreign = true;
    if (!on_device) {
        const size_t words = (size_t)n_peers * (size_t)stride;
        SPK_TRY(up.alloc(words + 1));
        if (words > 0) {
            SPK_HIP(hipMemcpyAsync(up.p, peer_labels, words * 4, hipMemcpyHostToDevice, ctx->stream));
            SPK_HIP(hipStreamSynchronize(ctx->stream));  // peer_labels is the caller's: done with it
        }
        S.rows = up.p;
    }
    const std::string bad = w + ": a peer label is greater than its own index (or >= n_nodes)";
    const std::string limit = w + ": no fixed point within 256 rounds";
    return cc_fixed_point(ctx, n_nodes, nullptr, nullptr, 0, lab, S, flags.p, count.p, SPK_E_INVALID, bad.c_str(),
                          limit.c_str(), T, out_rounds, out_n_clusters);
}

}  // namespace spk

using namespace spk;

extern "C" int spk_components(spk_ctx *ctx, int64_t *out_n_nodes, int64_t *out_n_clusters, int *out_rounds) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "spk_components: null ctx");
    SPK_HIP(hipSetDevice(ctx->device));
    ctx->comp.clear();  // whatever happens below, the previous labels are gone
    Components C;
    StageTimer T{ctx};
    DevBuf<uint32_t> eu, ev;
    int64_t n_nodes = 0;
    SPK_TRY(selection_edges(ctx, "spk_components", SPK_SEL_ALL, T, eu, ev, &n_nodes));
    SPK_TRY(build_components(ctx, n_nodes, ctx->sel.n, eu.p, ev.p, SPK_E_STATE,
                             "spk_components: a selected pair names a row outside its table", T, C));
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
    Components C;
    StageTimer T{ctx};
    DevBuf<uint32_t> eu, ev;
    SPK_TRY(eu.alloc((size_t)n_edges + 1));
    SPK_TRY(ev.alloc((size_t)n_edges + 1));
    if (n_edges > 0) {
        SPK_HIP(hipMemcpyAsync(eu.p, u, (size_t)n_edges * 4, hipMemcpyHostToDevice, ctx->stream));
        SPK_HIP(hipMemcpyAsync(ev.p, v, (size_t)n_edges * 4, hipMemcpyHostToDevice, ctx->stream));
        SPK_HIP(hipStreamSynchronize(ctx->stream));  // u / v are the caller's: done with them on every path below
    }
    SPK_TRY(build_components(ctx, n_nodes, n_edges, eu.p, ev.p, SPK_E_INVALID,
                             "spk_components_edges: a node id is >= n_nodes", T, C));
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

extern "C" int spk_components_copy_device(spk_ctx *ctx, int64_t start, int64_t count, uint32_t *d_out_label) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "spk_components_copy_device: null ctx");
    const Components &C = ctx->comp;
    SPK_REQUIRE(C.valid, SPK_E_STATE, "spk_components_copy_device: no components (run spk_components)");
    SPK_REQUIRE(start >= 0 && count >= 0 && start <= C.n_nodes && count <= C.n_nodes - start, SPK_E_INVALID,
                "spk_components_copy_device: range");
    SPK_REQUIRE(count == 0 || d_out_label, SPK_E_INVALID, "spk_components_copy_device: null out");
    if (!count) return SPK_OK;
    SPK_HIP(hipSetDevice(ctx->device));
    SPK_HIP(hipMemcpyAsync(d_out_label, C.label.p + start, (size_t)count * 4, hipMemcpyDeviceToDevice, ctx->stream));
    SPK_HIP(hipStreamSynchronize(ctx->stream));  // a collective on another stream reads it next
    return SPK_OK;
}

extern "C" int spk_components_merge(spk_ctx *ctx, int n_peers, const uint32_t *peer_labels, int64_t stride,
                                    int on_device, int64_t *out_n_clusters, int *out_rounds) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "spk_components_merge: null ctx");
    Components &C = ctx->comp;
    SPK_REQUIRE(C.valid, SPK_E_STATE, "spk_components_merge: no components (run spk_components)");
    SPK_TRY(merge_arguments("spk_components_merge", n_peers, peer_labels, stride, C.n_nodes));
    SPK_HIP(hipSetDevice(ctx->device));
    StageTimer T{ctx};
    int rounds = 0;
    int64_t n_clusters = 0;
    const int rc = merge_labels(ctx, "spk_components_merge", C.n_nodes, C.label.p, n_peers, peer_labels, stride,
                                on_device, T, &rounds, &n_clusters);
    if (rc != SPK_OK) {
        C.clear();  // some labels may be the union's already, others not: no components
        return rc;
    }
    C.n_clusters = n_clusters;
    C.rounds += rounds;
    if (C.ms >= 0.0 && T.result() >= 0.0) C.ms += T.result();
    else C.ms = -1.0;
    C.merged = true;
    if (out_n_clusters) *out_n_clusters = n_clusters;
    if (out_rounds) *out_rounds = rounds;
    return SPK_OK;
}

// ---- the sweep -------------------------------------------------------------------------------------------------------
extern "C" int spk_components_sweep(spk_ctx *ctx, int field, int n_thresholds, const double *thresholds,
                                    int64_t *out_n_nodes, int64_t *out_n_edges, int64_t *out_n_clusters,
                                    int *out_rounds) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "spk_components_sweep: null ctx");
    SPK_HIP(hipSetDevice(ctx->device));
    ctx->sweep.clear();  // whatever happens below, the previous sweep is gone
    SPK_REQUIRE(field == SPK_SEL_MP || field == SPK_SEL_TF_MP || field == SPK_SEL_ALL, SPK_E_INVALID,
                "spk_components_sweep: field is SPK_SEL_MP, SPK_SEL_TF_MP or SPK_SEL_ALL");
    int L = 0;
    SPK_TRY(sweep_thresholds("spk_components_sweep", field == SPK_SEL_ALL, n_thresholds, thresholds, &L));
    ComponentSweep W;
    StageTimer T{ctx};
    DevBuf<uint32_t> eu, ev;
    int64_t n_nodes = 0;
    SPK_TRY(selection_edges(ctx, "spk_components_sweep", field, T, eu, ev, &n_nodes));
    const Selection &S = ctx->sel;
    SPK_TRY(build_sweep(ctx, n_nodes, S.n, eu.p, ev.p, S.code.p, field == SPK_SEL_MP ? S.mpat.p : nullptr,
                        field == SPK_SEL_TF_MP ? S.tf_mp.p : nullptr, L, thresholds, SPK_E_STATE,
                        "spk_components_sweep: a selected pair names a row outside its table", T, W));
    ctx->sweep = std::move(W);
    if (out_n_nodes) *out_n_nodes = ctx->sweep.n_nodes;
    sweep_outputs(ctx->sweep, out_n_edges, out_n_clusters, out_rounds);
    return SPK_OK;
}

extern "C" int spk_components_sweep_edges(spk_ctx *ctx, int64_t n_nodes, int64_t n_edges, const uint32_t *u,
                                          const uint32_t *v, const double *score, int n_thresholds,
                                          const double *thresholds, int64_t *out_n_edges, int64_t *out_n_clusters,
                                          int *out_rounds) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "spk_components_sweep_edges: null ctx");
    SPK_HIP(hipSetDevice(ctx->device));
    ctx->sweep.clear();
    SPK_REQUIRE(n_nodes >= 0 && n_edges >= 0, SPK_E_INVALID, "spk_components_sweep_edges: negative count");
    SPK_REQUIRE(n_edges == 0 || (u && v), SPK_E_INVALID, "spk_components_sweep_edges: null edges");
    SPK_REQUIRE(n_thresholds == 0 || n_edges == 0 || score, SPK_E_INVALID, "spk_components_sweep_edges: null scores");
    SPK_REQUIRE(n_nodes <= (int64_t)UINT32_MAX, SPK_E_LIMIT, "spk_components_sweep_edges: more than 2^32 - 1 nodes");
    int L = 0;
    SPK_TRY(sweep_thresholds("spk_components_sweep_edges", n_thresholds == 0, n_thresholds, thresholds, &L));
    ComponentSweep W;
    StageTimer T{ctx};
    DevBuf<uint32_t> eu, ev;
    DevBuf<double> sc;
    const bool scored = n_thresholds > 0;
    SPK_TRY(eu.alloc((size_t)n_edges + 1));
    SPK_TRY(ev.alloc((size_t)n_edges + 1));
    SPK_TRY(sc.alloc((size_t)n_edges + 1));
    if (n_edges > 0) {
        SPK_HIP(hipMemcpyAsync(eu.p, u, (size_t)n_edges * 4, hipMemcpyHostToDevice, ctx->stream));
        SPK_HIP(hipMemcpyAsync(ev.p, v, (size_t)n_edges * 4, hipMemcpyHostToDevice, ctx->stream));
        if (scored) SPK_HIP(hipMemcpyAsync(sc.p, score, (size_t)n_edges * 8, hipMemcpyHostToDevice, ctx->stream));
        SPK_HIP(hipStreamSynchronize(ctx->stream));  // u / v / score are the caller's: done with them
    }
    SPK_TRY(build_sweep(ctx, n_nodes, n_edges, eu.p, ev.p, nullptr, nullptr, scored ? sc.p : nullptr, L, thresholds,
                        SPK_E_INVALID, "spk_components_sweep_edges: a node id is >= n_nodes", T, W));
    ctx->sweep = std::move(W);
    sweep_outputs(ctx->sweep, out_n_edges, out_n_clusters, out_rounds);
    return SPK_OK;
}

extern "C" int spk_components_sweep_copy(spk_ctx *ctx, int level, int64_t start, int64_t count, uint32_t *out_label) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "spk_components_sweep_copy: null ctx");
    const ComponentSweep &W = ctx->sweep;
    SPK_REQUIRE(W.valid, SPK_E_STATE, "spk_components_sweep_copy: no sweep (run spk_components_sweep)");
    SPK_REQUIRE(level >= 0 && level < W.levels, SPK_E_INVALID, "spk_components_sweep_copy: level");
    SPK_REQUIRE(start >= 0 && count >= 0 && start <= W.n_nodes && count <= W.n_nodes - start, SPK_E_INVALID,
                "spk_components_sweep_copy: range");
    SPK_REQUIRE(count == 0 || out_label, SPK_E_INVALID, "spk_components_sweep_copy: null out");
    if (!count) return SPK_OK;
    SPK_HIP(hipSetDevice(ctx->device));
    SPK_HIP(hipMemcpyAsync(out_label, W.label.p + (size_t)level * (size_t)W.n_nodes + (size_t)start, (size_t)count * 4,
                           hipMemcpyDeviceToHost, ctx->stream));
    SPK_HIP(hipStreamSynchronize(ctx->stream));
    return SPK_OK;
}

extern "C" int spk_components_sweep_info(spk_ctx *ctx, int *out_levels, int64_t *out_n_nodes, int64_t *out_n_edges,
                                         double *out_ms) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "spk_components_sweep_info: null ctx");
    const ComponentSweep &W = ctx->sweep;
    if (out_levels) *out_levels = W.valid ? W.levels : -1;
    if (out_n_nodes) *out_n_nodes = W.valid ? W.n_nodes : -1;
    if (out_n_edges) *out_n_edges = W.valid ? W.n_edges[W.levels - 1] : -1;
    if (out_ms) *out_ms = W.valid ? W.ms : -1.0;
    return SPK_OK;
}

extern "C" int spk_components_sweep_release(spk_ctx *ctx) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "spk_components_sweep_release: null ctx");
    SPK_HIP(hipSetDevice(ctx->device));
    SPK_HIP(hipStreamSynchronize(ctx->stream));
    ctx->sweep.clear();
    return SPK_OK;
}

extern "C" int spk_components_sweep_copy_device(spk_ctx *ctx, int level, int64_t start, int64_t count,
                                                uint32_t *d_out_label) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "spk_components_sweep_copy_device: null ctx");
    const ComponentSweep &W = ctx->sweep;
    SPK_REQUIRE(W.valid, SPK_E_STATE, "spk_components_sweep_copy_device: no sweep (run spk_components_sweep)");
    SPK_REQUIRE(level >= 0 && level < W.levels, SPK_E_INVALID, "spk_components_sweep_copy_device: level");
    SPK_REQUIRE(start >= 0 && count >= 0 && start <= W.n_nodes && count <= W.n_nodes - start, SPK_E_INVALID,
                "spk_components_sweep_copy_device: range");
    SPK_REQUIRE(count == 0 || d_out_label, SPK_E_INVALID, "spk_components_sweep_copy_device: null out");
    if (!count) return SPK_OK;
    SPK_HIP(hipSetDevice(ctx->device));
    SPK_HIP(hipMemcpyAsync(d_out_label, W.label.p + (size_t)level * (size_t)W.n_nodes + (size_t)start, (size_t)count * 4,
                           hipMemcpyDeviceToDevice, ctx->stream));
    SPK_HIP(hipStreamSynchronize(ctx->stream));  // a collective on another stream reads it next
    return SPK_OK;
}

extern "C" int spk_components_sweep_merge(spk_ctx *ctx, int level, int n_peers, const uint32_t *peer_labels,
                                          int64_t stride, int on_device, int64_t *out_n_clusters, int *out_rounds) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "spk_components_sweep_merge: null ctx");
    ComponentSweep &W = ctx->sweep;
    SPK_REQUIRE(W.valid, SPK_E_STATE, "spk_components_sweep_merge: no sweep (run spk_components_sweep)");
    SPK_REQUIRE(level >= 0 && level < W.levels, SPK_E_INVALID, "spk_components_sweep_merge: level");
    SPK_TRY(merge_arguments("spk_components_sweep_merge", n_peers, peer_labels, stride, W.n_nodes));
    SPK_HIP(hipSetDevice(ctx->device));
    W.merged = true;  // from here on the level's labels are no longer those of the stored edges
    W.m_level = -1;
    W.m_ms = -1.0;
    W.bridges.clear();  // they described the stored edges' own components
    StageTimer T{ctx};
    int rounds = 0;
    int64_t n_clusters = 0;
    const int rc = merge_labels(ctx, "spk_components_sweep_merge", W.n_nodes,
                                W.label.p + (size_t)level * (size_t)W.n_nodes, n_peers, peer_labels, stride, on_device,
                                T, &rounds, &n_clusters);
    if (rc != SPK_OK) {
        W.clear();  // some of the level's labels may be the union's already, others not: no sweep
        return rc;
    }
    W.n_clusters[level] = n_clusters;
    W.rounds[level] += rounds;
    if (W.ms >= 0.0 && T.result() >= 0.0) W.ms += T.result();
    else W.ms = -1.0;
    if (out_n_clusters) *out_n_clusters = n_clusters;
    if (out_rounds) *out_rounds = rounds;
    return SPK_OK;
}

extern "C" int spk_components_sweep_set_mode(spk_ctx *ctx, int mode) {
    SPK_REQUIRE(ctx && (mode == 0 || mode == 1), SPK_E_INVALID, "spk_components_sweep_set_mode: mode 0 or 1");
    ctx->sweep_mode = mode;
    return SPK_OK;
}

// ---- metrics of one level --------------------------------------------------------------------------------------------
extern "C" int spk_cluster_metrics(spk_ctx *ctx, int level, int64_t *out3) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "spk_cluster_metrics: null ctx");
    ComponentSweep &W = ctx->sweep;
    SPK_REQUIRE(W.valid, SPK_E_STATE, "spk_cluster_metrics: no sweep (run spk_components_sweep)");
    SPK_REQUIRE(level >= 0 && level < W.levels, SPK_E_INVALID, "spk_cluster_metrics: level");
    SPK_REQUIRE(!W.merged, SPK_E_STATE,
                "spk_cluster_metrics: a level of this sweep was merged with other shards' labels, and its stored "
                "edges are one shard's: the degrees would be partial");
    SPK_HIP(hipSetDevice(ctx->device));
    W.m_level = -1;  // whatever happens below, the previous level's metrics are gone
    W.m_ms = -1.0;
    hipStream_t st = ctx->stream;
    const int64_t n = W.n_nodes;
    DevBuf<unsigned long long> out;
    SPK_TRY(out.alloc(3));
    SPK_TRY(W.degree.alloc((size_t)n + 1));
    SPK_TRY(W.size.alloc((size_t)n + 1));
    SPK_TRY(W.max_degree.alloc((size_t)n + 1));
    SPK_TRY(W.degree_sum.alloc((size_t)n + 1));
    StageTimer T{ctx};
    SPK_TRY(T.open());
    SPK_HIP(hipMemsetAsync(out.p, 0, 3 * sizeof(unsigned long long), st));
    SPK_HIP(hipMemsetAsync(W.degree.p, 0, ((size_t)n + 1) * 4, st));
    SPK_HIP(hipMemsetAsync(W.size.p, 0, ((size_t)n + 1) * 4, st));
    SPK_HIP(hipMemsetAsync(W.max_degree.p, 0, ((size_t)n + 1) * 4, st));
    SPK_HIP(hipMemsetAsync(W.degree_sum.p, 0, ((size_t)n + 1) * 8, st));
    for (int k = 0; k <= level; ++k) {  // a level's range without its padding, whose (0, 0) would count for node 0
        if (!W.cnt[k]) continue;
        const unsigned g = cc_grid(ctx, W.cnt[k], CC_THREADS);
        const uint32_t *eu = W.eu.p + W.off[k], *ev = W.ev.p + W.off[k];
        if (ctx->metrics_edge_agg) k_cm_degree<true><<<g, CC_THREADS, 0, st>>>(W.cnt[k], eu, ev, W.degree.p);
        else k_cm_degree<false><<<g, CC_THREADS, 0, st>>>(W.cnt[k], eu, ev, W.degree.p);
        SPK_HIP(hipGetLastError());
    }
    const uint32_t *lab = W.label.p + (size_t)level * (size_t)n;
    const unsigned node_grid = cc_grid(ctx, n, CC_THREADS);
    if (n > 0) {
        k_cm_nodes<<<node_grid, CC_THREADS, 0, st>>>(n, lab, W.degree.p, W.size.p, W.degree_sum.p, W.max_degree.p);
        SPK_HIP(hipGetLastError());
        k_cm_scalars<<<node_grid, CC_THREADS, 0, st>>>(n, lab, W.size.p, out.p);
        SPK_HIP(hipGetLastError());
    }
    unsigned long long h[3] = {0, 0, 0};
    SPK_HIP(hipMemcpyAsync(h, out.p, sizeof(h), hipMemcpyDeviceToHost, st));
    SPK_TRY(T.close());
    W.m_level = level;
    W.m_ms = T.result();
    if (out3)
        for (int i = 0; i < 3; ++i) out3[i] = (int64_t)h[i];
    return SPK_OK;
}

extern "C" int spk_cluster_metrics_copy(spk_ctx *ctx, int64_t start, int64_t count, uint32_t *out_degree,
                                        uint32_t *out_size, uint64_t *out_degree_sum, uint32_t *out_max_degree) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "spk_cluster_metrics_copy: null ctx");
    const ComponentSweep &W = ctx->sweep;
    SPK_REQUIRE(W.valid && W.m_level >= 0, SPK_E_STATE, "spk_cluster_metrics_copy: no metrics (run spk_cluster_metrics)");
    SPK_REQUIRE(start >= 0 && count >= 0 && start <= W.n_nodes && count <= W.n_nodes - start, SPK_E_INVALID,
                "spk_cluster_metrics_copy: range");
    if (!count) return SPK_OK;
    SPK_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t s = (size_t)start, c = (size_t)count;
    if (out_degree) SPK_HIP(hipMemcpyAsync(out_degree, W.degree.p + s, c * 4, hipMemcpyDeviceToHost, st));
    if (out_size) SPK_HIP(hipMemcpyAsync(out_size, W.size.p + s, c * 4, hipMemcpyDeviceToHost, st));
    if (out_degree_sum) SPK_HIP(hipMemcpyAsync(out_degree_sum, W.degree_sum.p + s, c * 8, hipMemcpyDeviceToHost, st));
    if (out_max_degree) SPK_HIP(hipMemcpyAsync(out_max_degree, W.max_degree.p + s, c * 4, hipMemcpyDeviceToHost, st));
    SPK_HIP(hipStreamSynchronize(st));
    return SPK_OK;
}

extern "C" int spk_cluster_metrics_set_mode(spk_ctx *ctx, int mode) {
    SPK_REQUIRE(ctx && (mode == 0 || mode == 1), SPK_E_INVALID, "spk_cluster_metrics_set_mode: mode 0 or 1");
    ctx->metrics_edge_agg = mode == 1;
    return SPK_OK;
}

extern "C" int spk_cluster_metrics_info(spk_ctx *ctx, int *out_level, double *out_ms) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "spk_cluster_metrics_info: null ctx");
    const ComponentSweep &W = ctx->sweep;
    if (out_level) *out_level = W.valid ? W.m_level : -1;
    if (out_ms) *out_ms = W.valid && W.m_level >= 0 ? W.m_ms : -1.0;
    return SPK_OK;
}
