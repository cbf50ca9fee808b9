// Clusters against labels (gfx950): every level of the context's sweep scored against one truth id per node, the
// counts behind clusters.truth_table().  No counterpart in the reference release.
//
// The definitions (include/splink_hip.h) are exact integers over the labelled nodes: pairs inside a cluster (P), inside
// an entity (T) and inside both (tp), clusters that mix entities, entities split over clusters, entities recovered
// whole.  A cluster can hold 10^6 records, so nothing here adds per node onto per-cluster words; everything is read off
// sorted keys, and about ten integers per level leave the device.
//
// Once per call, over the n_nodes ids:
//   k_ag_ids     key = g << 1 | side for a labelled node (side = cross_only && v >= n_left), all ones for an unlabelled
//                one, which sorts last; value = the node; counts the labelled nodes M and the left ones; an id >= 2^31
//                only raises the flag the host reads before anything else runs.
//   sort         (key, node) pairs over 33 bits.  The first M places are the labelled nodes, entity after entity.
//   k_ag_heads, scan, k_ag_count<false>   below, with the entity in the cluster's place: the id runs give `entities`
//                and T; every place learns ent = the first place of its id's run, a dense name of the entity below
//                M, and the run's last place stores the entity's size at esize[ent] (one writer per entity).
// Per level k, over the M labelled places (the buffers are reused from level to level):
//   k_ag_keys    key = c_k[node] << (be + 1) | ent << 1 | side, be = the bits of M - 1.
//   sort         the keys over the bits in use (be + 1 + the bits of n_nodes - 1).
//   k_ag_heads   per place i of the sorted keys: (head_c ? i : 0, head_cg ? i : 0, left, left) -- head_c: the cluster
//                bits differ from place i - 1 (or i = 0), head_cg: the bits above the side bit differ.
//   scan         one inclusive scan of those records under (max, max, +, the later one's): start_c(i), start_cg(i) =
//                the first place of i's cluster run and of its (cluster, entity) run, the left places up to and
//                including i, and i's own left flag, so SL(i) = sl - left is the left places before i.
//   k_ag_count<true>   every counted pair inside a run is counted once, at its later place i: i - s(i) partners, or
//                under cross_only those of the other side, SL(i) - SL(s) for a right place and (i - s) - (SL(i) - SL(s))
//                for a left one; s = start_c gives P, s = start_cg gives tp.  A place is a head iff its start is itself:
//                the cluster heads are clusters_labelled; a (cluster, entity) head that is no cluster head and whose
//                predecessor still sits in its cluster's first run is the cluster's second run: clusters_mixed, once
//                per cluster.  The last place of a (cluster, entity) run knows the run's length: equal to esize[ent],
//                the entity lies in this one cluster (entities_split = entities - those); if the run is also the whole
//                cluster (it ends the cluster run and start_cg = start_c) the entity is recovered.
// That is one sort per level, not the two a second orientation (entity-major) would take: the entity's size, the only
// thing that orientation would add, is level-independent and is looked up at esize[ent].  Every labelled node is
// sorted at every level: leaving out the nodes that are the only labelled one of their cluster (they add no pair) took
// 0.3 ms (15%) off the device time at cfg2 and added 0.3 to 0.5 ms to the call's wall time, for the compaction's total
// has to reach the host at every level; it is not kept.
//
// Every kernel of this file is elementwise or a grid-stride reduction over a capped grid: registers -> wave (shuffles)
// -> workgroup (LDS) -> one 64-bit integer add per workgroup and non-zero field.  Integer adds do not depend on their
// arrival order, so two calls give the same bytes.  No workgroup waits for another: no spin, no ticket, no cooperative
// launch (rocprim's sort and scan are the library's).  Places are below M <= 2^31, offsets are 64-bit, sums are 64-bit:
// C(2^32 - 1, 2) < 2^63.  Every index a kernel forms is a start (<= its own place), a neighbour checked against M, an
// ent (a start of the entity pass, < M) or a node / label the sweep wrote (< n_nodes).
//
// Transient memory, freed at return: 8 (ids) + 24 (keys, nodes, both sorted) bytes per node, and per labelled node
// 8 (ent, esize) + 32 (the records and their scan); the level keys reuse the call's key buffers.  Plus rocprim's sort
// scratch.
#include <algorithm>

#include "spk_prim.h"

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "spk_agreement.hip targets gfx950 (MI355X) only"
#endif

namespace spk {

// One place per lane and trip: a workgroup step is AG_THREADS places.  The sums end in one global add per workgroup
// and field, all workgroups on the same few words, and those adds, not the streaming, were most of the reductions'
// time with 2048 workgroups of 256 threads (30 us per launch at 10^6 places): the same lanes as 512
// workgroups of 1024 issue a quarter of them.
constexpr int AG_THREADS = 1024;
constexpr int AG_WG_PER_CU = 2;   // capped grid, the workgroups stride over the places (as the components' kernels)
constexpr int AG_ACC = 6;         // sums of one count launch: cluster heads, P, tp, mixed, entities whole, recovered
constexpr uint64_t AG_NULL_KEY = ~0ull;
constexpr int64_t AG_MAX_NODES = (int64_t)1 << 31;  // cluster, entity and side then fit 31 + 31 + 1 key bits

struct alignas(16) AgRun {
    uint32_t c, cg;  // in: the place if it heads a cluster / (cluster, entity) run, else 0; scanned: the run's start
    uint32_t sl;     // in: 1 for a left place (cross_only); scanned: the left places up to and including this one
    uint32_t left;   // this place's own flag (the scan keeps the later operand's)
};
struct AgRunOp {
    __host__ __device__ AgRun operator()(const AgRun &a, const AgRun &b) const {
        return AgRun{a.c > b.c ? a.c : b.c, a.cg > b.cg ? a.cg : b.cg, a.sl + b.sl, b.left};
    }
};

// out[f] += the workgroup's sum of x[f].  Every thread of the workgroup calls it, once per kernel.
template <int N>
__device__ inline void ag_block_add(unsigned long long (&x)[N], unsigned long long *out) {
    __shared__ unsigned long long s[AG_THREADS / 64][N];
#pragma unroll
    for (int f = 0; f < N; ++f)
        for (int off = 32; off > 0; off >>= 1) x[f] += __shfl_down(x[f], off, 64);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int f = 0; f < N; ++f) s[threadIdx.x >> 6][f] = x[f];
    __syncthreads();
    if (threadIdx.x < N) {
        unsigned long long t = 0;
        for (int w = 0; w < AG_THREADS / 64; ++w) t += s[w][threadIdx.x];
        if (t) (void)__hip_atomic_fetch_add(out + threadIdx.x, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// count[0] += the labelled nodes, count[1] += those of the left side
__global__ __launch_bounds__(AG_THREADS) void k_ag_ids(int64_t n_nodes, const int64_t *__restrict__ ids, int64_t n_left,
                                                       int cross, uint64_t *__restrict__ key,
                                                       uint32_t *__restrict__ node, unsigned long long *count,
                                                       unsigned int *bad) {
    unsigned long long x[2] = {0ull, 0ull};
    const int64_t step = (int64_t)gridDim.x * AG_THREADS;
    for (int64_t v = (int64_t)blockIdx.x * AG_THREADS + threadIdx.x; v < n_nodes; v += step) {
        const int64_t g = ids[v];
        uint64_t k = AG_NULL_KEY;
        if (g > (int64_t)INT32_MAX) {
            *bad = 1u;
        } else if (g >= 0) {
            const uint64_t side = cross && v >= n_left ? 1ull : 0ull;
            k = (uint64_t)g << 1 | side;
            x[0] += 1ull;
            x[1] += 1ull - side;
        }
        key[v] = k;
        node[v] = (uint32_t)v;
    }
    ag_block_add<2>(x, count);
}

__global__ __launch_bounds__(AG_THREADS) void k_ag_keys(int64_t M, const uint32_t *__restrict__ node,
                                                        const uint32_t *__restrict__ ent,
                                                        const uint32_t *__restrict__ label, int64_t n_left, int cross,
                                                        int sh_c, uint64_t *__restrict__ key) {
    const int64_t step = (int64_t)gridDim.x * AG_THREADS;
    for (int64_t j = (int64_t)blockIdx.x * AG_THREADS + threadIdx.x; j < M; j += step) {
        const uint32_t v = node[j];
        const uint64_t side = cross && (int64_t)v >= n_left ? 1ull : 0ull;
        key[j] = (uint64_t)label[(size_t)v] << sh_c | (uint64_t)ent[j] << 1 | side;
    }
}

__global__ __launch_bounds__(AG_THREADS) void k_ag_heads(int64_t M, const uint64_t *__restrict__ skey, int sh_c, int cross,
                                                         AgRun *__restrict__ out) {
    const int64_t step = (int64_t)gridDim.x * AG_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * AG_THREADS + threadIdx.x; i < M; i += step) {
        const uint64_t k = skey[i], p = i ? skey[i - 1] : 0ull;
        const bool hc = i == 0 || (k >> sh_c) != (p >> sh_c), hcg = i == 0 || (k >> 1) != (p >> 1);
        const uint32_t left = cross && !(k & 1ull) ? 1u : 0u;
        out[i] = AgRun{hc ? (uint32_t)i : 0u, hcg ? (uint32_t)i : 0u, left, left};
    }
}

// LEVEL = false, the entity pass: ent[i] = the start of i's run, esize[start] = the run's length.  LEVEL = true: reads
// them (ent from the key, through ent_mask).  acc [AG_ACC].
template <bool LEVEL>
__global__ __launch_bounds__(AG_THREADS) void k_ag_count(int64_t M, const uint64_t *__restrict__ skey,
                                                         const AgRun *__restrict__ st, int cross, uint64_t ent_mask,
                                                         uint32_t *ent, uint32_t *esize, unsigned long long *acc) {
    unsigned long long x[AG_ACC] = {};
    const int64_t step = (int64_t)gridDim.x * AG_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * AG_THREADS + threadIdx.x; i < M; i += step) {
        const AgRun a = st[i];
        const int64_t sc = a.c, scg = a.cg;
        int64_t pc = i - sc, pcg = i - scg;
        if (cross) {
            const AgRun b = st[sc], d = st[scg];
            const int64_t sl = (int64_t)a.sl - a.left;  // the left places before i, before sc, before scg
            const int64_t lc = sl - ((int64_t)b.sl - b.left), lcg = sl - ((int64_t)d.sl - d.left);
            pc = a.left ? pc - lc : lc;
            pcg = a.left ? pcg - lcg : lcg;
        }
        x[0] += sc == i ? 1ull : 0ull;
        x[1] += (unsigned long long)pc;
        x[2] += (unsigned long long)pcg;
        if (scg == i && sc != i) {  // i >= 1, and i - 1 lies in the same cluster
            const AgRun p = st[i - 1];
            x[3] += p.cg == p.c ? 1ull : 0ull;
        }
        const bool last = i + 1 == M;
        AgRun nx = a;
        if (!last) nx = st[i + 1];
        if (last || (int64_t)nx.cg == i + 1) {  // i ends its (cluster, entity) run
            const uint32_t len = (uint32_t)(i - scg + 1);
            if (LEVEL) {
                if (esize[(size_t)((skey[i] >> 1) & ent_mask)] == len) {
                    x[4] += 1ull;
                    x[5] += (last || (int64_t)nx.c == i + 1) && scg == sc ? 1ull : 0ull;
                }
            } else {
                esize[(size_t)scg] = len;
            }
        }
        if (!LEVEL) ent[i] = (uint32_t)scg;
    }
    ag_block_add<AG_ACC>(x, acc);
}

static unsigned ag_grid(const spk_ctx *ctx, int64_t items) {
    const int64_t g = (items + AG_THREADS - 1) / AG_THREADS;
    return (unsigned)std::max<int64_t>(std::min<int64_t>(g, AG_WG_PER_CU * (int64_t)ctx->n_cu), 1);
}

static int ag_bits(int64_t largest) {  // bits that hold 0 .. largest, at least one
    int b = 1;
    while (b < 63 && (largest >> b)) ++b;
    return b;
}

struct AgBuffers {
    DevBuf<uint64_t> key, skey;
    DevBuf<uint32_t> node, snode, ent, esize;
    DevBuf<AgRun> head, run;
    DevBuf<uint8_t> tmp;
};

// heads, scan and counts over the first M places of B.skey
template <bool LEVEL>
static int ag_count_sorted(spk_ctx *ctx, AgBuffers &B, int64_t M, int sh_c, int cross, uint64_t ent_mask,
                           unsigned long long *acc) {
    hipStream_t st = ctx->stream;
    const unsigned g = ag_grid(ctx, M);
    k_ag_heads<<<g, AG_THREADS, 0, st>>>(M, B.skey.p, sh_c, cross, B.head.p);
    SPK_HIP(hipGetLastError());
    SPK_TRY(inclusive_scan_op(st, B.tmp, B.head.p, B.run.p, M, AgRunOp()));
    k_ag_count<LEVEL><<<g, AG_THREADS, 0, st>>>(M, B.skey.p, B.run.p, cross, ent_mask, B.ent.p, B.esize.p, acc);
    SPK_HIP(hipGetLastError());
    return SPK_OK;
}

}  // namespace spk

using namespace spk;

extern "C" int spk_cluster_agreement(spk_ctx *ctx, const int64_t *ids, int64_t n_left, int cross_only, int64_t *out) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "spk_cluster_agreement: null ctx");
    const ComponentSweep &W = ctx->sweep;
    SPK_REQUIRE(W.valid, SPK_E_STATE, "spk_cluster_agreement: no sweep (run spk_components_sweep)");
    const int64_t n = W.n_nodes;
    const int L = W.levels, cross = cross_only != 0;
    SPK_REQUIRE(out, SPK_E_INVALID, "spk_cluster_agreement: null out");
    SPK_REQUIRE(n == 0 || ids, SPK_E_INVALID, "spk_cluster_agreement: null ids");
    SPK_REQUIRE(!cross || (n_left >= 0 && n_left <= n), SPK_E_INVALID, "spk_cluster_agreement: n_left outside [0, n_nodes]");
    SPK_REQUIRE(n <= AG_MAX_NODES, SPK_E_LIMIT, "spk_cluster_agreement: more than 2^31 nodes");
    SPK_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    // everything below lives for this call only
    AgBuffers B;
    DevBuf<int64_t> wide;
    DevBuf<unsigned long long> acc;  // [labelled, labelled left | AG_ACC of the entity pass | AG_ACC per level]
    DevBuf<unsigned int> bad;
    const size_t n_acc = 2 + (size_t)AG_ACC * (size_t)(L + 1);
    std::vector<unsigned long long> h(n_acc, 0ull);
    StageTimer T{ctx};
    SPK_TRY(acc.alloc(n_acc));
    SPK_TRY(bad.alloc(1));
    SPK_HIP(hipMemsetAsync(acc.p, 0, n_acc * sizeof(unsigned long long), st));
    SPK_HIP(hipMemsetAsync(bad.p, 0, sizeof(unsigned int), st));
    int64_t M = 0, M_left = 0;
    if (n > 0) {
        SPK_TRY(wide.alloc((size_t)n));
        SPK_TRY(B.key.alloc((size_t)n));
        SPK_TRY(B.skey.alloc((size_t)n));
        SPK_TRY(B.node.alloc((size_t)n));
        SPK_TRY(B.snode.alloc((size_t)n));
        // the upload is no launch: outside the interval.  ids is borrowed until the close below.
        SPK_HIP(hipMemcpyAsync(wide.p, ids, (size_t)n * 8, hipMemcpyHostToDevice, st));
        SPK_TRY(T.open());
        k_ag_ids<<<ag_grid(ctx, n), AG_THREADS, 0, st>>>(n, wide.p, n_left, cross, B.key.p, B.node.p, acc.p, bad.p);
        SPK_HIP(hipGetLastError());
        unsigned int h_bad = 0u;
        SPK_TRY(T.stop());
        SPK_HIP(hipMemcpyAsync(&h_bad, bad.p, sizeof(h_bad), hipMemcpyDeviceToHost, st));
        SPK_HIP(hipMemcpyAsync(h.data(), acc.p, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        SPK_HIP(hipStreamSynchronize(st));
        SPK_TRY(T.add());
        SPK_REQUIRE(h_bad == 0u, SPK_E_INVALID, "spk_cluster_agreement: a truth id of 2^31 or more");
        M = (int64_t)h[0];
        M_left = (int64_t)h[1];
    }
    if (M > 0) {
        SPK_TRY(B.ent.alloc((size_t)M));
        SPK_TRY(B.esize.alloc((size_t)M));
        SPK_TRY(B.head.alloc((size_t)M));
        SPK_TRY(B.run.alloc((size_t)M));
        const int be = ag_bits(M - 1), sh_c = be + 1, n_bits = sh_c + ag_bits(n - 1);
        const uint64_t ent_mask = ((uint64_t)1 << be) - 1;
        SPK_TRY(T.open());
        // the entity pass: a valid key is below 2^32 and the NULL key has bit 32 set
        SPK_TRY(sort_pairs_u64(st, B.tmp, B.key.p, B.skey.p, B.node.p, B.snode.p, n, 33));
        SPK_TRY(ag_count_sorted<false>(ctx, B, M, 1, cross, 0, acc.p + 2));
        const unsigned g = ag_grid(ctx, M);
        for (int k = 0; k < L; ++k) {
            const uint32_t *lab = W.label.p + (size_t)k * (size_t)n;
            k_ag_keys<<<g, AG_THREADS, 0, st>>>(M, B.snode.p, B.ent.p, lab, n_left, cross, sh_c, B.key.p);
            SPK_HIP(hipGetLastError());
            SPK_TRY(sort_keys_u64(st, B.tmp, B.key.p, B.skey.p, M, n_bits));
            SPK_TRY(ag_count_sorted<true>(ctx, B, M, sh_c, cross, ent_mask, acc.p + 2 + (size_t)AG_ACC * (size_t)(k + 1)));
        }
        SPK_TRY(T.stop());  // the read-back is no launch
        SPK_HIP(hipMemcpyAsync(h.data(), acc.p, n_acc * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        SPK_HIP(hipStreamSynchronize(st));
        SPK_TRY(T.add());
    }
    const unsigned long long *e = h.data() + 2;  // the entity pass: [0] entities, [1] T
    const int64_t M_right = M - M_left;
    const int64_t total = cross ? M_left * M_right : M * (M - 1) / 2;  // M <= 2^31
    for (int k = 0; k < L; ++k) {
        const unsigned long long *a = e + (size_t)AG_ACC * (size_t)(k + 1);
        int64_t *o = out + (size_t)k * SPK_AGREE_FIELDS;
        o[0] = M;
        o[1] = (int64_t)a[0];
        o[2] = (int64_t)e[0];
        o[3] = (int64_t)a[1];
        o[4] = (int64_t)e[1];
        o[5] = (int64_t)a[2];
        o[6] = (int64_t)a[3];
        o[7] = (int64_t)(e[0] - a[4]);
        o[8] = (int64_t)a[5];
        o[9] = total;
    }
    ctx->agree_levels = L;
    ctx->agree_ms = T.result();
    return SPK_OK;
}

extern "C" int spk_cluster_agreement_info(spk_ctx *ctx, int *out_levels, double *out_ms) {
    SPK_REQUIRE(ctx, SPK_E_INVALID, "spk_cluster_agreement_info: null ctx");
    if (out_levels) *out_levels = ctx->agree_levels;
    if (out_ms) *out_ms = ctx->agree_ms;
    return SPK_OK;
}
