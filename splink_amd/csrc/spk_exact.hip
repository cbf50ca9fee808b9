// The exact phase of the comparison pass: everything that runs over the work lists the filter wrote.  List sizing
// and compaction (k_prefix, k_compact, k_compact_lev), the exact passes (k_gamma_exact, k_gamma_exact_simple,
// k_lev_refill), the slow, rest and huge passes over what they leave, and the launch logic of the phase
// (enqueue_phase, enqueue_slow, run_huge: the interface in spk_gamma.h).
#include <algorithm>

#include "spk_gamma.h"
#include "spk_interp.h"

namespace spk {

// The exact passes run over column k's compacted work list -- every region's undecided pairs back
// to back (k_compact) -- with a grid-stride loop, so every CU gets the same share of cells however
// unevenly they fall over the regions (a region of one large block can hold several times the
// average).  Block b of k_compact copies region b's list to its prefix offset.
//
// The lists are sized on the device, so the pass needs no host round trip between the filter and
// the exact kernels: k_prefix scans the region counts of every column (one workgroup) into
// xpref[k][b] and xinfo = [col_base[K] | col_count[K] | overflow | total].  Column k's list
// starts at xlist + col_base[k]; its slow-pass list (a subset) at the same offset in the second
// half of xlist.  If the lists exceed the capacity, `overflow` makes every exact kernel a no-op
// and the host re-runs the phase with room for `total` (codes are untouched until then).
constexpr int PFX_THREADS = 1024;
constexpr int PFX_PER = 8;  // region counts a k_prefix thread keeps in registers
__global__ __launch_bounds__(PFX_THREADS) void k_prefix(const unsigned int *__restrict__ region_count, int K,
                                                        int n_regions, int64_t cap, int64_t *__restrict__ xpref,
                                                        int64_t *__restrict__ xinfo, unsigned long long *__restrict__ done) {
    // One workgroup per column (blockIdx.x): wave-level inclusive scans (shuffles) and one scan of the
    // 16 wave totals, two barriers.  A thread's counts (<= PFX_PER of them, 5 at 20 regions per CU)
    // stay in registers.  The last workgroup to finish (device-scope counter) lays the columns' lists
    // out one after another and flags an overflow of `cap`.
    constexpr int NW = PFX_THREADS / 64;
    __shared__ int64_t wsum[NW];
    __shared__ bool s_last;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int per = (n_regions + PFX_THREADS - 1) / PFX_THREADS;
    const int b0 = threadIdx.x * per;
    const bool in_regs = per <= PFX_PER;  // block-uniform
    const int k = blockIdx.x;
    const unsigned int *rc = region_count + (int64_t)k * n_regions;
    unsigned int cur[PFX_PER];
    int64_t mine = 0;
    if (in_regs) {
#pragma unroll
        for (int q = 0; q < PFX_PER; ++q) {
            cur[q] = (q < per && b0 + q < n_regions) ? rc[b0 + q] : 0u;
            mine += cur[q];
        }
    } else {
        for (int b = b0; b < b0 + per && b < n_regions; ++b) mine += rc[b];
    }
    int64_t v = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int64_t t = __shfl_up(v, off, 64);
        if (lane >= off) v += t;
    }
    if (lane == 63) wsum[wave] = v;
    __syncthreads();
    if (wave == 0) {
        int64_t w = lane < NW ? wsum[lane] : 0;
#pragma unroll
        for (int off = 1; off < NW; off <<= 1) {
            const int64_t t = __shfl_up(w, off, 64);
            if (lane >= off) w += t;
        }
        if (lane < NW) wsum[lane] = w;
    }
    __syncthreads();
    int64_t acc = v - mine + (wave > 0 ? wsum[wave - 1] : 0);  // exclusive
    int64_t *pf = xpref + (int64_t)k * (n_regions + 1);
    if (in_regs) {
#pragma unroll
        for (int q = 0; q < PFX_PER; ++q) {
            if (q < per && b0 + q < n_regions) pf[b0 + q] = acc;
            acc += cur[q];
        }
    } else {
        for (int b = b0; b < b0 + per && b < n_regions; ++b) {
            pf[b] = acc;
            acc += rc[b];
        }
    }
    if (threadIdx.x == 0) {
        const int64_t tot = wsum[NW - 1];
        pf[n_regions] = tot;
        xinfo[K + k] = tot;
        __threadfence();
        s_last = atomicAdd(done, 1ull) == (unsigned long long)(K - 1);
    }
    __syncthreads();
    if (s_last && threadIdx.x == 0) {
        __threadfence();
        int64_t base = 0;
        for (int c = 0; c < K; ++c) {
            xinfo[c] = base;
            base += (int64_t)atomicAdd(reinterpret_cast<unsigned long long *>(&xinfo[K + c]), 0ull);  // from L2
        }
        xinfo[2 * K] = base > cap ? 1 : 0;
        xinfo[2 * K + 1] = base;
        *done = 0;  // ready for a re-run of the phase
    }
}

__device__ inline int64_t exact_count(const GammaArgs &A, const int64_t *xinfo, int k) {
    return xinfo[2 * A.K] ? 0 : xinfo[A.K + k];
}

__global__ void k_compact(GammaArgs A, ColSet cs, const int64_t *__restrict__ xpref, int32_t *__restrict__ xlist,
                          const int64_t *__restrict__ xinfo) {
    if (xinfo[2 * A.K]) return;  // overflow: the host re-runs the phase
    const int k = cs.k[blockIdx.y];
    const int64_t *pref = xpref + (int64_t)k * (A.n_regions + 1);
    const Region R = my_region(A);
    const int32_t *src = region_list(A, k, R);
    const int64_t n = A.region_count[(int64_t)k * A.n_regions + blockIdx.x];
    int32_t *dst = xlist + xinfo[k] + pref[blockIdx.x];
    // four entries per thread in flight before their stores (a long region's copy is latency-bound otherwise)
    const int64_t bd = blockDim.x;
    for (int64_t i = threadIdx.x; i < n; i += 4 * bd) {
        int32_t v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = i + u * bd < n ? src[i + u * bd] : 0;
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (i + u * bd < n) dst[i + u * bd] = v[u];
    }
}

// Levenshtein tests of the `<=` / `<` kind need the distance only up to the largest value any of them
// accepts (the cut), so the bit-parallel scans stop as soon as the distance provably exceeds it.
__device__ inline int simple_lev_cut(const SimpleCol &sc, int ncp_a, int ncp_b) {
    const double den = (double)(ncp_a + ncp_b) / 2.0;
    int cut = 0;
    for (int i = 0; i < sc.n_tests; ++i) {
        if (sc.op[i] != SPK_OP_LEV && sc.op[i] != SPK_OP_LEVRATIO) continue;
        if (sc.cmp[i] != SPK_CMP_LE && sc.cmp[i] != SPK_CMP_LT) return 1 << 30;
        // every v > bound fails `v cmp t` (resp. `v / den cmp t`): one unit of margin over t * den
        const double lim = sc.op[i] == SPK_OP_LEV ? sc.t[i] : sc.t[i] * den;
        if (!(lim < 1e9)) return 1 << 30;
        const int bound = lim < 0.0 ? 0 : (int)floor(lim) + 1;
        cut = bound > cut ? bound : cut;
    }
    return cut;
}

// lev_cell's level of a cell from eq (1 equal / 0 unequal) and the clamped distance; nsum = na + nb.
__device__ inline int lev_level_of(const SimpleCol &sc, int eq, int lev, int nsum) {
    const double den = (double)nsum / 2.0;
    for (int i = 0; i < sc.n_tests; ++i) {
        const int op = sc.op[i], cmp = sc.cmp[i];
        int r;
        if (op == SPK_OP_STR_CMP) r = ((eq == 1) == (cmp == SPK_CMP_EQ)) ? KT : KF;
        else if (op == SPK_OP_LEVRATIO && den == 0.0) r = KN;
        else r = op == SPK_OP_LEV ? cmpd((double)lev, sc.t[i], cmp) : cmpd((double)lev / den, sc.t[i], cmp);
        if (r == KT) return sc.level[i];
    }
    return sc.else_level;
}

// Upper bound on the multiset intersection of two rows from their character-bag rows (k_bag_rows), or -1 when
// a bucket is saturated on both sides.  Σ min(a, b) = (Σ a + Σ b - Σ |a - b|) / 2 over the nibbles, spread to
// bytes (v_sad_u8 sums four absolute byte differences).
__device__ inline int bag_inter_ub(const uint4 &a0, const uint4 &a1, const uint4 &b0, const uint4 &b1) {
    const uint32_t wa[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w & 0xFFFFu};
    const uint32_t wb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w & 0xFFFFu};
    uint32_t sad = 0, sa = 0, sb = 0, sat = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const uint32_t la = wa[q] & 0x0F0F0F0Fu, ha = (wa[q] >> 4) & 0x0F0F0F0Fu;
        const uint32_t lb = wb[q] & 0x0F0F0F0Fu, hb = (wb[q] >> 4) & 0x0F0F0F0Fu;
        sad = __builtin_amdgcn_sad_u8(la, lb, sad);
        sad = __builtin_amdgcn_sad_u8(ha, hb, sad);
        sa = __builtin_amdgcn_sad_u8(la, 0u, sa);
        sa = __builtin_amdgcn_sad_u8(ha, 0u, sa);
        sb = __builtin_amdgcn_sad_u8(lb, 0u, sb);
        sb = __builtin_amdgcn_sad_u8(hb, 0u, sb);
        const uint32_t t = wa[q] & wb[q];
        sat |= t & (t >> 1) & (t >> 2) & (t >> 3) & 0x11111111u;
    }
    if (sat) return -1;
    const int oa = (int)((a1.w >> 16) & 0xFFu), ob = (int)((b1.w >> 16) & 0xFFu);
    return (int)((sa + sb - sad) / 2u) + (oa < ob ? oa : ob);
}

// k_compact for a Levenshtein column: a listed cell whose rows' bag distance already exceeds the cut is decided
// here (its level is lev_cell's for any distance past the cut), one with a row past 64 units goes straight to
// the slow list; the others are packed to the front of the
// region's slice of the list in order, and the slice's tail is -1, which the exact passes skip (whole waves of
// it, mostly).  0.206 ms per cfg5 call (round 5); four cells per thread per round (their loads in flight together)
// took 0.260, and unordered packing through one LDS counter per workgroup (no barriers) 0.210.  Round 6 sorts the
// slow cells (0.272 ms) and pipelines the loads across rounds (0.242 ms, profiles/r6_ab_compact_lev_pipeline.log).
constexpr int CL_THREADS = 256;
constexpr int CL_SLOW = 1024;  // LDS buffer of slow-list cells per workgroup
__global__ __launch_bounds__(CL_THREADS) void k_compact_lev(GammaArgs A, int k, int si, const int64_t *__restrict__ xpref,
                                                            int32_t *__restrict__ xlist, const int64_t *__restrict__ xinfo) {
    if (xinfo[2 * A.K]) return;  // overflow: the host re-runs the phase
    __shared__ SimpleCol s_sc;
    __shared__ int s_kept[CL_THREADS / 64];
    __shared__ int32_t s_slow[CL_SLOW];
    __shared__ uint8_t s_skey[CL_SLOW];     // the buffered slow cells' shorter row length (sort key)
    __shared__ uint16_t s_srank[CL_SLOW];   // rank of each among the cells of its key
    __shared__ unsigned int s_sbin[3 * 64];  // counting-sort bins (keys 0 .. 128)
    __shared__ int s_ns;
    __shared__ unsigned int s_sbase;
    if (threadIdx.x == 0) {
        s_sc = A.simple[si];
        s_ns = 0;
    }
    __syncthreads();
    const SimpleCol &sc = s_sc;
    const int64_t *pref = xpref + (int64_t)k * (A.n_regions + 1);
    const Region R = my_region(A);
    const int32_t *src = region_list(A, k, R);
    const int64_t n = A.region_count[(int64_t)k * A.n_regions + blockIdx.x];
    int32_t *dst = xlist + xinfo[k] + pref[blockIdx.x];
    const uint4 *bag0 = A.cols0[sc.col].bag, *bag1 = A.cols1[sc.col].bag;
    const uint32_t stride = (uint32_t)sc.stride;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int32_t *slow_list = A.slow + A.slow_off[k];
    // The buffered slow cells to the slow list (one device atomic), in order of their shorter row's length: the
    // 128-bit pass runs a wave as long as its slowest lane, and cells of similar lengths scan similarly long
    // (host simulation over cfg5's bag-filtered slow cells: lane utilisation 0.53 -> 0.60 sorted per 1,024 cells).
    // A counting sort through LDS: one LDS atomic per cell, a 192-bin scan in wave 0, one scatter.
    auto flush_slow = [&]() {
        const int c = s_ns;
        if (threadIdx.x == 0) s_sbase = atomicAdd(A.slow_count + k, (unsigned int)c);
        if (threadIdx.x < 3 * 64) s_sbin[threadIdx.x] = 0;
        __syncthreads();
        for (int j = threadIdx.x; j < c; j += CL_THREADS) s_srank[j] = (uint16_t)atomicAdd(&s_sbin[s_skey[j]], 1u);
        __syncthreads();
        if (threadIdx.x < 64) {  // wave 0: exclusive scan, three bins per lane
            const int t = threadIdx.x;
            const unsigned int a = s_sbin[3 * t], b = s_sbin[3 * t + 1], d = s_sbin[3 * t + 2];
            unsigned int v = a + b + d;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned int u = __shfl_up(v, off, 64);
                if (t >= off) v += u;
            }
            const unsigned int ex = v - a - b - d;
            s_sbin[3 * t] = ex;
            s_sbin[3 * t + 1] = ex + a;
            s_sbin[3 * t + 2] = ex + a + b;
        }
        __syncthreads();
        for (int j = threadIdx.x; j < c; j += CL_THREADS) slow_list[s_sbase + s_sbin[s_skey[j]] + s_srank[j]] = s_slow[j];
        __syncthreads();
        if (threadIdx.x == 0) s_ns = 0;
    };
    int64_t kept = 0;  // block-uniform
    // software pipeline: the next round's pair rows and the list entry after that are in flight with this
    // round's bag rows, so a round waits on one memory round trip instead of three
    int32_t pc = 0, xc = 0, yc = 0;
    if (threadIdx.x < n) {
        pc = src[threadIdx.x];
        xc = A.pl[pc];
        yc = A.pr[pc];
    }
    int32_t pn = threadIdx.x + CL_THREADS < n ? src[threadIdx.x + CL_THREADS] : 0;
    for (int64_t i0 = 0; i0 < n; i0 += CL_THREADS) {
        const int64_t i = i0 + threadIdx.x;
        // unconditional loads at clamped indices (pair 0's rows, the list's last entry), no branch around them:
        // this round's bag rows, the next round's pair rows, the list entry after that
        const uint4 a0 = bag0[2 * (int64_t)xc], a1 = bag0[2 * (int64_t)xc + 1];
        const uint4 b0 = bag1[2 * (int64_t)yc], b1 = bag1[2 * (int64_t)yc + 1];
        const int64_t i2 = i + CL_THREADS, i3 = i2 + CL_THREADS;
        const int32_t p2 = i2 < n ? pn : 0;
        const int32_t x2 = A.pl[p2], y2 = A.pr[p2];
        pn = src[i3 < n ? i3 : n - 1];
        __builtin_amdgcn_sched_barrier(0);  // all issued before the first wait
        // the bound before any branch on the rows' lengths, so no load is sunk into one (two round trips)
        const int la = (int)(a1.w >> 24), lb = (int)(b1.w >> 24);
        int inter = bag_inter_ub(a0, a1, b0, b1);
        bool keep = false, slow = false;
        const int32_t p = pc;
        int skey = 0;
        if (i < n) {
            keep = true;
            if (la != 255 && lb != 255) {
                // a row past 64 units has no 64-bit planes: the exact pass would only pass the cell on to the
                // 128-bit slow pass, after loading its rows -- it goes to the slow list from here
                slow = la > 64 || lb > 64;
                skey = la < lb ? la : lb;  // <= 128: rows with bag rows have at most 128 units
                if (inter >= 0) {
                    const int mn = la < lb ? la : lb, mx = la < lb ? lb : la;
                    inter = inter < mn ? inter : mn;
                    const int cut = simple_lev_cut(sc, la, lb);
                    if (mx - inter > cut) {  // unequal rows (a positive bag distance), distance past the cut
                        code_add_atomic(A, p, (uint32_t)(lev_level_of(sc, 0, cut + 1, la + lb) + 1) * stride);
                        keep = slow = false;
                    }
                }
            }
        }
        const unsigned long long ms = __ballot(keep && slow);
        if (ms) {  // into the workgroup's LDS buffer (the device counter once per CL_SLOW cells: a shared
                   // counter per wave serialised, 2.9 ms per cfg5 call)
            int sb = 0;
            if (lane == 0) sb = atomicAdd(&s_ns, __popcll(ms));
            sb = __shfl(sb, 0);
            if (keep && slow) {
                const int q = sb + __popcll(ms & ((1ull << lane) - 1ull));
                s_slow[q] = p;
                s_skey[q] = (uint8_t)skey;
            }
            keep = keep && !slow;
        }
        const unsigned long long m = __ballot(keep);
        if (lane == 0) s_kept[wv] = __popcll(m);
        __syncthreads();
        int off = 0, tot = 0;
#pragma unroll
        for (int q = 0; q < CL_THREADS / 64; ++q) {
            off += q < wv ? s_kept[q] : 0;
            tot += s_kept[q];
        }
        if (keep) dst[kept + off + __popcll(m & ((1ull << lane) - 1ull))] = p;
        kept += tot;
        if (s_ns > CL_SLOW - CL_THREADS || i0 + CL_THREADS >= n) flush_slow();  // block-uniform (after the barrier)
        __syncthreads();
        pc = p2;
        xc = x2;
        yc = y2;
    }
    for (int64_t i = kept + threadIdx.x; i < n; i += CL_THREADS) dst[i] = -1;
}

// Exact pass over column k through the interpreter.  SET: eval_pred's (spk_interp.h).
template <bool SET>
__device__ __forceinline__ void gamma_exact_body(const GammaArgs &A, int k, const int32_t *xlist, const int64_t *xinfo) {
    const int64_t n = exact_count(A, xinfo, k);
    const int32_t *items = xlist + xinfo[k];
    const int64_t stride = (int64_t)gridDim.x * X_THREADS;
    for (int64_t base = (int64_t)blockIdx.x * X_THREADS; base < n; base += stride) {  // block-uniform
        const int64_t i = base + threadIdx.x;
        bool to_slow = false;
        int32_t p = 0;
        if (i < n) {
            p = items[i];
            int level = 0;
            const int st = eval_column<M_EXACT, SET>(A, k, A.pl[p], A.pr[p], level);
            if (st == ST_DONE) code_add(A, p, (uint32_t)(level + 1) * (uint32_t)A.stride[k]);
            else to_slow = true;
        }
        wave_append(A.slow + A.slow_off[k], A.slow_count + k, to_slow, p);
    }
}
__global__ __launch_bounds__(X_THREADS) void k_gamma_exact(GammaArgs A, int k, const int32_t *xlist,
                                                            const int64_t *xinfo) {
    gamma_exact_body<false>(A, k, xlist, xinfo);
}
__global__ __launch_bounds__(X_THREADS) void k_gamma_exact_set(GammaArgs A, int k, const int32_t *xlist,
                                                                const int64_t *xinfo) {
    gamma_exact_body<true>(A, k, xlist, xinfo);
}

// Per len_l + len_r (S < S_MAX): the scan's cut and each test's largest passing distance for unequal strings
// (the filter's integer forms: lev_a, the host's ratio tables), and *tab = 1 when every test is a `<=` / `<` on
// the distance or a string (in)equality, so a cell's level is a table lookup.  Callers barrier after it.
template <int S_MAX, int CUT_MAX>
__device__ inline void lev_tables(const GammaArgs &A, const SimpleCol &sc, uint8_t *s_cut, int16_t (*s_bp)[MAX_TESTS],
                                  int *tab) {
    static_assert(S_MAX <= THR_S, "every len_l + len_r of a 64-bit scan is inside the host's ratio tables");
    for (int S = threadIdx.x; S < S_MAX; S += X_THREADS) {  // blocks of X_THREADS
        const int c = simple_lev_cut(sc, S, 0);
        s_cut[S] = (uint8_t)(c < CUT_MAX ? c : CUT_MAX);
        for (int i = 0; i < sc.n_tests; ++i) {
            int bp = -1;
            if (sc.op[i] == SPK_OP_STR_CMP) bp = sc.cmp[i] == SPK_CMP_EQ ? -1 : CUT_MAX + 1;
            else if (sc.op[i] == SPK_OP_LEV) bp = sc.lev_a[i];
            else if (sc.thr_off[i] >= 0) bp = A.thr[sc.thr_off[i] + S];
            s_bp[S][i] = (int16_t)(bp < -1 ? -1 : (bp > CUT_MAX + 1 ? CUT_MAX + 1 : bp));
        }
    }
    if (threadIdx.x == 0) {
        int ok = 1;
        for (int i = 0; i < sc.n_tests; ++i) {
            const int op = sc.op[i];
            if (op == SPK_OP_LEV) ok &= (sc.tflag[i] & (TF_GE | TF_EXACT)) ? 0 : 1;
            else if (op == SPK_OP_LEVRATIO) ok &= sc.thr_off[i] >= 0 ? 1 : 0;
            else ok &= op == SPK_OP_STR_CMP ? 1 : 0;
        }
        *tab = ok;
    }
}

// 1 equal, 0 unequal, -1 needs the units (hash match on rows without dictionary ids).
__device__ inline int meta_equal(const RecMeta &a, const RecMeta &b) {
    if (a.cpf & b.cpf & CPF_ID) return a.key == b.key ? 1 : 0;
    const bool keyed = ((a.cpf | b.cpf) & CPF_ID) == 0;
    if (a.len16 != b.len16 || a.head != b.head || (keyed && a.key != b.key)) return 0;
    return a.len16 <= 4 ? 1 : -1;
}

// Exact pass cell of a simple string column (the template shapes): the tests run straight on the two
// rows' records, bit-planes and units -- no interpreter, no re-evaluation of the NULL / equality
// branches the filter pass already settled, each similarity computed at most once.
__device__ int simple_exact(const SimpleCol &sc, const ColDesc &c0, const ColDesc &c1, int32_t x, int32_t y,
                            int &level) {
    uint64_t pa[N_PLANES], pb[N_PLANES];
    const RecMeta ma = c0.meta[x], mb = c1.meta[y];
    if (ma.len16 < 0 || mb.len16 < 0) {
        level = sc.null_level;
        return ST_DONE;
    }
    const StrView a = row_view(c0, ma, x, sc.col), b = row_view(c1, mb, y, sc.col);
    int eq = meta_equal(ma, mb);
    if (eq < 0) eq = units_equal(a, b) ? 1 : 0;
    double jw = -1.0;
    int lev = -1;
    for (int i = 0; i < sc.n_tests; ++i) {
        const int op = sc.op[i], cmp = sc.cmp[i];
        const double t = sc.t[i];
        int r;
        if (op == SPK_OP_STR_CMP) {
            r = ((eq == 1) == (cmp == SPK_CMP_EQ)) ? KT : KF;
        } else if (op == SPK_OP_JW) {
            if (jw < 0.0) {
                if (eq == 1) jw = a.n > 0 ? 1.0 : 0.0;
                else if (a.n > 64 || b.n > 64) return ST_NEEDS_SLOW;
                else jw = jw_exact(a, b);
            }
            r = cmpd(jw, t, cmp);
        } else {  // SPK_OP_LEV / SPK_OP_LEVRATIO
            const double den = (double)(a.ncp + b.ncp) / 2.0;
            if (op == SPK_OP_LEVRATIO && den == 0.0) {
                r = KN;
            } else {
                if (lev < 0) {
                    if (eq == 1) lev = 0;
                    else if (a.n > 64 || b.n > 64 || a.ncp != a.n || b.ncp != b.n) return ST_NEEDS_SLOW;
                    else if (a.planes && b.planes) {
#pragma unroll
                        for (int q = 0; q < N_PLANES; ++q) {
                            pa[q] = a.planes[q];
                            pb[q] = b.planes[q];
                        }
                        lev = lev_rows_planes(pa, a.n, pb, b.n, simple_lev_cut(sc, a.ncp, b.ncp), sc.np);
                    } else {
                        lev = lev_exact(a, b, simple_lev_cut(sc, a.ncp, b.ncp));
                    }
                }
                r = op == SPK_OP_LEV ? cmpd((double)lev, t, cmp) : cmpd((double)lev / den, t, cmp);
            }
        }
        if (r == KT) {
            level = sc.level[i];
            return ST_DONE;
        }
    }
    level = sc.else_level;
    return ST_DONE;
}

// Exact pass cell of a Jaro-Winkler template column (every test `jaro_winkler_sim > / >= t`): the JW
// code alone, so its kernel keeps a small register budget (X_JW).
__device__ int jw_cell(const SimpleCol &sc, const ColDesc &c0, const ColDesc &c1, int32_t x, int32_t y, int &level) {
    const RecMeta ma = c0.meta[x], mb = c1.meta[y];
    if (ma.len16 < 0 || mb.len16 < 0) {
        level = sc.null_level;
        return ST_DONE;
    }
    const StrView a = row_view(c0, ma, x, sc.col), b = row_view(c1, mb, y, sc.col);
    int eq = meta_equal(ma, mb);
    if (eq < 0) eq = units_equal(a, b) ? 1 : 0;
    double jw;
    if (eq == 1) jw = a.n > 0 ? 1.0 : 0.0;
    else if (a.n > 64 || b.n > 64) return ST_NEEDS_SLOW;
    else jw = jw_exact(a, b);
    for (int i = 0; i < sc.n_tests; ++i) {
        if (cmpd(jw, sc.t[i], sc.cmp[i]) == KT) {
            level = sc.level[i];
            return ST_DONE;
        }
    }
    level = sc.else_level;
    return ST_DONE;
}

// Exact pass cell of a Levenshtein-class template column (tests: `=` / `<>`, levenshtein [ratio]):
// both rows' bit-planes are loaded in the same round trip as the records and the distance comes
// from them alone (lev_rows_planes).  Rows without planes (> 64 units or a unit >= 256) go to the
// global-memory pass.  A kernel of its own, so its register budget is not the JW path's.
// The column descriptors come from LDS, so their pointers are generic: the records and planes are read through
// global-address-space views (global_load, not flat -- a flat load also counts against lgkmcnt, so every wait on
// it waits for the LDS reads too).
typedef const __attribute__((address_space(1))) uint64_t GU64;
__device__ __attribute__((always_inline)) inline RecMeta load_meta_global(const RecMeta *m, int64_t row) {
    static_assert(sizeof(RecMeta) == 32, "RecMeta: four 8-byte words");
    GU64 *q = (GU64 *)(m + row);
    uint64_t w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = q[i];
    RecMeta out;
    __builtin_memcpy(&out, w, sizeof(out));
    return out;
}
// cutt / bpt: lev_tables' per len_l + len_r cut and thresholds for a 64-bit scan (nullptr: the tests one by one)
__device__ int lev_cell(const SimpleCol &sc, const ColDesc &c0, const ColDesc &c1, int32_t x, int32_t y, int &level,
                        const uint8_t *cutt = nullptr, const int16_t (*bpt)[MAX_TESTS] = nullptr) {
    uint64_t pa[N_PLANES], pb[N_PLANES];
    {
        GU64 *qa = (GU64 *)(c0.planes + (int64_t)x * N_PLANES);
        GU64 *qb = (GU64 *)(c1.planes + (int64_t)y * N_PLANES);
#pragma unroll
        for (int i = 0; i < N_PLANES; ++i) {
            pa[i] = qa[i];
            pb[i] = qb[i];
        }
    }
    const RecMeta ma = load_meta_global(c0.meta, x), mb = load_meta_global(c1.meta, y);
    if (ma.len16 < 0 || mb.len16 < 0) {
        level = sc.null_level;
        return ST_DONE;
    }
    int eq = meta_equal(ma, mb);
    if (eq < 0) eq = units_equal(row_view(c0, ma, x, sc.col), row_view(c1, mb, y, sc.col)) ? 1 : 0;
    const int na = meta_cplen(ma), nb = meta_cplen(mb);
    const bool planes = (ma.cpf & mb.cpf & CPF_PLANES) != 0;
    int lev = -1;
    for (int i = 0; i < sc.n_tests; ++i) {
        const int op = sc.op[i], cmp = sc.cmp[i];
        const double t = sc.t[i];
        int r;
        if (op == SPK_OP_STR_CMP) {
            r = ((eq == 1) == (cmp == SPK_CMP_EQ)) ? KT : KF;
        } else {
            const double den = (double)(na + nb) / 2.0;
            if (op == SPK_OP_LEVRATIO && den == 0.0) {
                r = KN;
            } else {
                if (lev < 0) {
                    if (eq == 1) lev = 0;
                    else if (!planes) return ST_NEEDS_SLOW;
                    else {
                        const int S = na + nb;  // <= 128: rows of <= 64 units
                        lev = lev_rows_planes(pa, ma.len16, pb, mb.len16, bpt != nullptr ? (int)cutt[S] : simple_lev_cut(sc, na, nb),
                                              sc.np);
                        if (bpt != nullptr) {  // levels by table: the tests before this one failed for eq = 0 too
                            int lv = sc.else_level;
                            for (int j = sc.n_tests - 1; j >= 0; --j) lv = lev <= bpt[S][j] ? sc.level[j] : lv;
                            level = lv;
                            return ST_DONE;
                        }
                    }
                }
                r = op == SPK_OP_LEV ? cmpd((double)lev, t, cmp) : cmpd((double)lev / den, t, cmp);
            }
        }
        if (r == KT) {
            level = sc.level[i];
            return ST_DONE;
        }
    }
    level = sc.else_level;
    return ST_DONE;
}

// The Levenshtein variant is latency-bound (record + plane loads per cell): it keeps registers to
// LEV_WAVES waves per SIMD so enough cells are in flight.
// Work bins of a Levenshtein cell: the scan runs over the shorter row (trip count) with a word as
// wide as the longer one needs, and a wave runs as long as its slowest lane and at the widest word
// any lane needs.  So each workgroup's 256 cells are regrouped by (longer > 32 units, shorter length)
// before they are evaluated: lanes of a wave then get similar trip counts and most waves stay at
// 32-bit words.  Only the assignment of cells to lanes changes; every cell is evaluated once, as
// before.  Cells with a row past 64 units (no 64-bit planes: the 128-bit slow pass takes them) get bins
// of their own, 128 + shorter length, so their waves hold no cell the exact pass evaluates and they
// reach the slow list sorted by that pass's trip count.  Bin LEV_BINS - 1 also holds the empty slots
// past the end of the list.
constexpr int LEV_BINS = 192;
__device__ inline int lev_work_bin(int la, int lb) {
    if (la < 0 || lb < 0) return 0;  // a NULL row: lev_cell settles it at once (not the slow list)
    const int mn = la < lb ? la : lb, mx = la < lb ? lb : la;
    return (mx > 64 ? 128 : (mx > 32 ? 64 : 0)) + (mn < 63 ? mn : 63);
}

// Counting sort of the workgroup's (key, item) by key through LDS: one LDS atomic per lane, a
// LEV_BINS exclusive scan in wave 0 (three bins per lane), one scatter and one gather.  Three barriers.
__device__ inline void lev_sort_items(int &key, bool &have, int32_t &p, int32_t &x, int32_t &y) {
    __shared__ unsigned int s_bin[LEV_BINS];
    __shared__ int32_t s_p[X_THREADS], s_x[X_THREADS], s_y[X_THREADS];
    __shared__ uint8_t s_have[X_THREADS], s_key[X_THREADS];
    const int t = threadIdx.x;
    if (t < LEV_BINS) s_bin[t] = 0;
    __syncthreads();
    const unsigned int r = atomicAdd(&s_bin[key], 1u);
    __syncthreads();
    static_assert(LEV_BINS == 3 * 64, "lev_sort_items scans three bins per lane");
    if (t < 64) {  // wave 0: three bins per lane
        const unsigned int a = s_bin[3 * t], b = s_bin[3 * t + 1], c = s_bin[3 * t + 2];
        unsigned int v = a + b + c;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned int u = __shfl_up(v, off, 64);
            if (t >= off) v += u;
        }
        const unsigned int ex = v - a - b - c;
        s_bin[3 * t] = ex;
        s_bin[3 * t + 1] = ex + a;
        s_bin[3 * t + 2] = ex + a + b;
    }
    __syncthreads();
    const unsigned int pos = s_bin[key] + r;
    s_p[pos] = p;
    s_x[pos] = x;
    s_y[pos] = y;
    s_have[pos] = have ? 1 : 0;
    s_key[pos] = (uint8_t)key;
    __syncthreads();
    p = s_p[t];
    x = s_x[t];
    y = s_y[t];
    have = s_have[t] != 0;
    key = s_key[t];
}

#ifndef SPK_LEV_WAVES
#define SPK_LEV_WAVES 4
#endif
constexpr int LEV_WAVES = SPK_LEV_WAVES;
// The Jaro-Winkler variant keeps its full register budget (138 VGPRs, 3 waves per SIMD): capped at
// 4 waves (128 VGPRs, 40 B of spills) it measured the same on MI355X (52.1 vs 52.3 us per call).
constexpr int JW_WAVES = 1;
// The JW-only cells (jw_cell) take 120 VGPRs: 4 waves per SIMD, twice the workgroups the generic kernel keeps resident.
constexpr int JWC_WAVES = 4;
// Columns of one exact launch: blocks [c g, (c + 1) g) work through column si[c]'s list, so the
// short Jaro-Winkler lists of several columns share one launch (and its tail).
struct ExactCols {
    int n;
    int g;  // blocks per column
    int si[4];
    int k[4], col[4];  // the columns' code positions and table columns (= simple[si].k / .col): the
                       // list bounds and the column descriptors load in one round, not after simple[si]
};

// Diagnostic build only (-DSPK_X_STAMPS): per-workgroup start / end wall-clock stamps (100 MHz) of the JW
// exact launch and the number of cells each workgroup evaluated, read with spk_debug_x_stamps
// (tools/ab_x_stamps.py).
#ifdef SPK_X_STAMPS
constexpr int X_STAMP_BLOCKS = 16384;
__device__ unsigned long long g_x_stamps[5 * X_STAMP_BLOCKS];
#endif
// MODE: X_GENERIC (simple_exact: any simple string column), X_LEV (lev_cell), X_JW (jw_cell).  Each mode
// is its own kernel so its register budget is that of its own cell code: simple_exact carries the
// Levenshtein scans too, and at its 190 VGPRs the JW cells ran 2 waves per SIMD.
enum XMode : int { X_GENERIC = 0, X_LEV = 1, X_JW = 2 };
template <int MODE, int XW = (MODE == X_LEV ? LEV_WAVES : (MODE == X_JW ? JWC_WAVES : JW_WAVES))>
__global__ __launch_bounds__(X_THREADS, XW) void k_gamma_exact_simple(GammaArgs A, ExactCols C,
                                                                   const int32_t *xlist, const int64_t *xinfo) {
    __shared__ SimpleCol s_sc;
    __shared__ ColDesc s_c0, s_c1;
    constexpr int XS_MAX = MODE == X_LEV ? 129 : 1;  // len_l + len_r of 64-bit rows, plus one
    __shared__ uint8_t s_cut[XS_MAX];
    __shared__ int16_t s_bp[XS_MAX][MAX_TESTS];
    __shared__ int s_tab;
#ifdef SPK_X_STAMPS
    unsigned long long x_t0 = wall_clock64(), x_cells = 0, x_t1 = 0, x_t2 = 0;
#endif
    const int col_slot = (int)(blockIdx.x / (unsigned)C.g);  // block-uniform
    const int64_t bid = (int64_t)blockIdx.x - (int64_t)col_slot * C.g;
    int si = C.si[0], k = C.k[0], colx = C.col[0];
#pragma unroll
    for (int c = 1; c < 4; ++c)
        if (c == col_slot) {
            si = C.si[c];
            k = C.k[c];
            colx = C.col[c];
        }
    // one round of independent loads: the column's descriptors (thread 0), the list bounds and every
    // thread's first item and pair rows
    if (threadIdx.x == 0) {
        s_sc = A.simple[si];
        s_c0 = A.cols0[colx];
        s_c1 = A.cols1[colx];
    }
    const int64_t n = exact_count(A, xinfo, k);
    const int32_t *items = xlist + xinfo[k];
    const int64_t stride = (int64_t)C.g * X_THREADS;
    // software pipeline: the next item's pair rows (and, for Levenshtein, the rows' lengths) are in
    // flight while this one is evaluated, and the list entry after that one is read a round earlier still, so
    // the pair-row loads of the next item never wait on its list entry (one memory round trip per cell, shared
    // with the current cell's records and planes)
    int64_t i = bid * X_THREADS + threadIdx.x;
    int32_t p = -1, x = 0, y = 0, key = LEV_BINS - 1;  // p = -1: no cell (past the list, or a k_compact_lev slot)
    if (i < n) {
        p = items[i];
        x = A.pl[p < 0 ? 0 : p];
        y = A.pr[p < 0 ? 0 : p];
    }
    int32_t pn = i + stride < n ? items[i + stride] : -1;  // the next item's list entry
    __syncthreads();
#ifdef SPK_X_STAMPS
    x_t1 = wall_clock64();
#endif
    const SimpleCol &sc = s_sc;
    constexpr bool LEV = MODE == X_LEV;
    if constexpr (LEV) {
        lev_tables<XS_MAX, XS_MAX - 2>(A, sc, s_cut, s_bp, &s_tab);
        __syncthreads();
    }
    const bool tab = LEV && s_tab != 0;  // block-uniform
    // Regroup by work bin only in free-text columns (rows past 64 units, so planes_hi exists): there the
    // trip counts spread widely (cfg5 addresses: 2.98 -> 2.67 ms per call).  In short-string columns
    // the sort's barriers cost more than it saves (cfg2 email: 475 -> 505 us), so they keep the old order.
    const bool regroup = LEV && s_c0.planes_hi != nullptr && s_c1.planes_hi != nullptr;  // block-uniform
    if (regroup && p >= 0) key = lev_work_bin(s_c0.meta[x].len16, s_c1.meta[y].len16);
    for (int64_t base = bid * X_THREADS; base < n; base += stride) {  // block-uniform
        bool have = p >= 0;
        const int64_t i2 = i + stride;
        // unconditional loads (clamped indices: pair 0 and the list's last entry are read harmlessly), so no
        // divergent branch makes the compiler wait on the loads in flight
        const int32_t p2 = i2 < n ? pn : -1;
        const int32_t q2 = p2 < 0 ? 0 : p2;
        const int32_t x2 = A.pl[q2], y2 = A.pr[q2];
        int32_t key2 = LEV_BINS - 1;
        if (regroup && p2 >= 0) key2 = lev_work_bin(s_c0.meta[x2].len16, s_c1.meta[y2].len16);
        const int64_t i3 = i2 + stride;
        const int32_t pn3 = items[i3 < n ? i3 : n - 1];
        pn = i3 < n ? pn3 : -1;
        if (regroup) lev_sort_items(key, have, p, x, y);
        bool to_slow = false;
        if (have && regroup && key >= 128) {
            // a row past 64 units (work bins 128 +): no 64-bit planes, the 128-bit slow pass takes the cell --
            // straight to its list, without loading the rows' planes and records first
            to_slow = true;
        } else if (have) {
            int level = 0;
            int st;
            if constexpr (MODE == X_LEV)
                st = lev_cell(sc, s_c0, s_c1, x, y, level, s_cut, tab ? s_bp : nullptr);
            else if constexpr (MODE == X_JW) st = jw_cell(sc, s_c0, s_c1, x, y, level);
            else st = simple_exact(sc, s_c0, s_c1, x, y, level);
#ifdef SPK_X_STAMPS
            if (x_t2 == 0) x_t2 = wall_clock64() + (unsigned long long)(level & 0);
#endif
            if (st != ST_DONE) to_slow = true;
            else if (C.n > 1) code_add_atomic(A, p, (uint32_t)(level + 1) * (uint32_t)sc.stride);
            else code_add(A, p, (uint32_t)(level + 1) * (uint32_t)sc.stride);
        }
        wave_append(A.slow + A.slow_off[k], A.slow_count + k, to_slow, p);
#ifdef SPK_X_STAMPS
        x_cells += have ? 1 : 0;
#endif
        i = i2;
        p = p2;
        x = x2;
        y = y2;
        key = key2;
    }
#ifdef SPK_X_STAMPS
    if (MODE == X_JW && threadIdx.x == 0 && blockIdx.x < X_STAMP_BLOCKS) {
        g_x_stamps[5 * blockIdx.x] = x_t0;
        g_x_stamps[5 * blockIdx.x + 1] = wall_clock64();
        g_x_stamps[5 * blockIdx.x + 2] = x_cells;
        g_x_stamps[5 * blockIdx.x + 3] = x_t1;
        g_x_stamps[5 * blockIdx.x + 4] = x_t2;
    }
#endif
}
#ifdef SPK_X_STAMPS
extern "C" int spk_debug_x_stamps(uint64_t *out, int n) {
    SPK_HIP(hipDeviceSynchronize());
    SPK_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_x_stamps), sizeof(uint64_t) * (size_t)std::min(n, 5 * X_STAMP_BLOCKS)));
    return SPK_OK;
}
#endif

// ---- Levenshtein exact pass with lane refill from a per-wave queue ----------------------------------------------
// In k_gamma_exact_simple<X_LEV> one lane scans one cell and a wave runs as long as its slowest lane: nearly every
// wave of 64 cells holds one that runs to the end (a pair within the cut) while most stop early, so a wave ran
// ~2-3x the mean trip count (tools/lev_refill_sim.py over the synthetic data: cfg5 addresses 12.8 steps per cell
// on average with the diagonal exit, 39 for the slowest of 64; cfg2 emails 7.5 vs 14.6).  Here a lane that
// finishes takes another cell, so a wave's steps follow the mean:
//   - batch: all 64 lanes set up the next 64 cells of the wave's range at once (full SIMD width, as the per-lane
//     kernel does): NULL / equal / length-gap / empty-remainder cells finish there, cells with a row past 64
//     units or a unit >= 256 go to the slow list, and the rest -- stripped planes, lengths, cut -- go into the
//     wave's LDS queue.  The batch runs when the queue is empty; its rows' records and planes were loaded by the
//     previous batch (three-stage prefetch: list entries, row ids, records + planes), and it is the only place
//     the loop touches global memory, so no wait in the loop waits on a load issued less than a batch ago;
//   - round (every LEVQ_STEPS scan steps): finished cells' levels (table lookups, no fp64) go to an LDS result
//     buffer (written as code adds at the next batch), and idle lanes take queued cells (LDS reads) when
//     LEVQ_ADOPT or more are idle or few lanes still scan;
//   - step: 32-bit words when every scanning lane's pattern has <= 32 units, else 64-bit; the text bit of
//     step j is read from the fixed text planes (bfe).  Early exit on the end cell's diagonal (D[j + m - n][j] >
//     cut proves the distance > cut: values never decrease along a diagonal), tested every LEVQ_STEPS steps.
// Levels are lev_cell's: the same tests in the same order on the same (cut + 1 clamped) distance.
constexpr int LEVQ_WAVES = 4;       // waves per SIMD (VGPR budget 128; the NP = 8 form takes 3)
#ifndef SPK_LEVQ_ADOPT
#define SPK_LEVQ_ADOPT 16
#endif
#ifndef SPK_LEVQ_STEPS
#define SPK_LEVQ_STEPS 2
#endif
constexpr int LEVQ_ADOPT = SPK_LEVQ_ADOPT;  // idle lanes that trigger a hand-out while many lanes still scan
constexpr int LEVQ_STEPS = SPK_LEVQ_STEPS;  // scan steps between rounds
static_assert(32 % LEVQ_STEPS == 0, "k_lev_refill moves a text's upper plane words down between blocks, at j = 32");
constexpr int LEVQ_WG_PER_CU = 4;

// Diagnostic build only (-DSPK_LEVQ_STATS): per-launch totals of k_lev_refill's schedule (tools/ab_lev_refill.py
// prints them): waves, batches, rounds, hand-out rounds, wave-steps by word width, lane-steps, cells scanned,
// cycles in batches / in steps / in the whole loop.
#ifdef SPK_LEVQ_STATS
__device__ unsigned long long g_levq[16];
#define LEVQ_STAT(i, v) (st_[i] += (unsigned long long)(v))
#else
#define LEVQ_STAT(i, v) ((void)0)
#endif

// One 64-bit word per plane row: the pass scans rows of <= 64 units (cells the filter listed); cells with a longer
// or non-Latin-1 row go on to the slow list.
template <int NP>
__global__ __launch_bounds__(X_THREADS, NP == 8 ? 3 : LEVQ_WAVES) void k_lev_refill(GammaArgs A, int si, int32_t *xlist,
                                                                                   const int64_t *xinfo) {
    typedef uint64_t Word;
    constexpr int WPB = X_THREADS / 64;
    constexpr int PW = 2;             // 32-bit words per plane row
    constexpr int QP = 2 * PW * NP;   // queue words of the pattern and text planes
    constexpr int QW = QP + 2;        // + p, m | n | cut | nsum
    constexpr int S_MAX = 128 + 1;    // len_l + len_r of rows this pass scans, plus one
    constexpr int CUT_MAX = 128 - 1;  // distances here are <= 64: a larger cut is no cut
    __shared__ SimpleCol s_sc;
    __shared__ ColDesc s_c0, s_c1;
    __shared__ uint32_t s_q[WPB][QW][64];
    __shared__ int32_t s_slow[WPB][128];
    __shared__ uint32_t s_res[WPB][2][128];      // finished cells: p, code delta
    __shared__ int16_t s_bp[S_MAX][MAX_TESTS];  // largest clamped distance passing test i (eq = 0), -1 none
    __shared__ uint8_t s_cut[S_MAX];
    __shared__ int s_tab;
    if (threadIdx.x == 0) {
        s_sc = A.simple[si];
        s_c0 = A.cols0[s_sc.col];
        s_c1 = A.cols1[s_sc.col];
    }
    __syncthreads();
    const SimpleCol &sc = s_sc;
    lev_tables<S_MAX, CUT_MAX>(A, sc, s_cut, s_bp, &s_tab);
    __syncthreads();
    const bool tab = s_tab != 0;
    const int k = sc.k, n_tests = sc.n_tests;
    const uint32_t stride = (uint32_t)sc.stride;
    auto level_of = [&](int lev, int S) -> int {  // eq = 0
        if (!tab) return lev_level_of(sc, 0, lev, S);
        int level = sc.else_level;
        for (int i = n_tests - 1; i >= 0; --i) level = lev <= s_bp[S][i] ? sc.level[i] : level;
        return level;
    };
    // the input list and where the cells this pass cannot scan go
    const int64_t n_items = exact_count(A, xinfo, k);
    const int32_t *items = xlist + xinfo[k];
    int32_t *out_list = A.slow + A.slow_off[k];
    unsigned int *out_count = A.slow_count + k;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    // the wave's contiguous range of batches (64 list entries each)
    const int64_t n_batches = (n_items + 63) / 64;
    const int64_t n_waves = (int64_t)gridDim.x * WPB;
    const int64_t per = (n_batches + n_waves - 1) / n_waves;
    const int64_t w = (int64_t)blockIdx.x * WPB + wv;
    const int64_t b_end = (w + 1) * per < n_batches ? (w + 1) * per : n_batches;
    int64_t bn = w * per < b_end ? w * per : b_end;  // wave-uniform: next batch to set up
    if (bn >= b_end) return;  // whole waves only: no barrier follows
    // global-address-space views of the rows' records and planes (global_load, not flat: a flat load also
    // counts against lgkmcnt, so the LDS reads after it would wait for the gather)
    typedef const __attribute__((address_space(1))) uint32_t GWord;
    typedef const __attribute__((address_space(1))) uint64_t GPlane;
    // (read through the kernel-argument pointers, so they stay in scalar registers)
    const int colx = A.simple[si].col;
    GWord *meta0 = (GWord *)A.cols0[colx].meta, *meta1 = (GWord *)A.cols1[colx].meta;
    GPlane *plane0 = (GPlane *)A.cols0[colx].planes, *plane1 = (GPlane *)A.cols1[colx].planes;
    // list entry of this lane in batch b, clamped into the range (unconditional loads: no divergent skips)
    auto entry = [&](int64_t b) -> int32_t {
        const int64_t bb = b < b_end ? b : b_end - 1;
        int64_t i = bb * 64 + lane;
        i = i < n_items ? i : n_items - 1;
        return items[i];
    };
    // staged batch: records (key, len16, head, cpf) and planes 0 .. NP - 1 of both rows
    uint32_t ska = 0, skb = 0, sfa = 0, sfb = 0;
    int32_t sla = 0, slb = 0;
    uint64_t sha = 0, shb = 0;
    uint64_t sqa[NP], sqb[NP];
#pragma unroll
    for (int b = 0; b < NP; ++b) sqa[b] = sqb[b] = 0;
    auto stage = [&](int32_t x, int32_t y) {
        GWord *ma = meta0 + (int64_t)x * 8, *mb = meta1 + (int64_t)y * 8;
        ska = ma[0];
        sla = (int32_t)ma[1];
        sha = ((uint64_t)ma[5] << 32) | ma[4];
        sfa = ma[7];
        skb = mb[0];
        slb = (int32_t)mb[1];
        shb = ((uint64_t)mb[5] << 32) | mb[4];
        sfb = mb[7];
        GPlane *qa = plane0 + (int64_t)x * N_PLANES, *qb = plane1 + (int64_t)y * N_PLANES;
#pragma unroll
        for (int b = 0; b < NP; ++b) {
            sqa[b] = qa[b];
            sqb[b] = qb[b];
        }
    };
    // prefetch pipeline: p0 = entry(bn) with its rows staged, p1 = entry(bn + 1) with row ids x1 / y1, p2 =
    // entry(bn + 2)
    // (-1: a cell k_compact_lev decided; its loads read pair 0 harmlessly)
    auto pair_of = [](int32_t q) { return q < 0 ? 0 : q; };
    int32_t p0 = entry(bn), p1 = entry(bn + 1), p2 = entry(bn + 2);
    int32_t x1 = A.pl[pair_of(p1)], y1 = A.pr[pair_of(p1)];
    stage(A.pl[pair_of(p0)], A.pr[pair_of(p0)]);
    int q_head = 0, q_count = 0, n_res = 0, n_slow = 0;  // wave-uniform
#ifdef SPK_LEVQ_STATS
    unsigned long long st_[16] = {};
    const unsigned long long t_loop = clock64();
#endif
    // the lane's cell: `active` while it holds one, `run` while its scan has text units left
    bool active = false, run = false;
    int32_t p = 0;
    uint32_t P[PW * NP], T[PW * NP];  // plane b: words [PW b, PW b + PW) of the pattern / text planes
#pragma unroll
    for (int b = 0; b < PW * NP; ++b) P[b] = T[b] = 0;
    Word VP = 0, VN = 0;
    int m = 1, n = 0, j = 0, cut = 0, S = 0;
    auto flush_res = [&]() {  // the buffered code adds (fire-and-forget atomics)
        for (int i = lane; i < n_res; i += 64) code_add_atomic(A, (int32_t)s_res[wv][0][i], s_res[wv][1][i]);
        n_res = 0;
    };
    auto flush_slow = [&](int cnt) {  // the first cnt (<= 64) buffered cells to the output list
        unsigned int base = 0;
        if (lane == 0) base = atomicAdd(out_count, (unsigned int)cnt);
        base = __shfl(base, 0);
        if (lane < cnt) out_list[base + lane] = s_slow[wv][lane];
        const int rest = n_slow - cnt;
        const int32_t moved = lane < rest ? s_slow[wv][cnt + lane] : 0;
        __builtin_amdgcn_wave_barrier();
        if (lane < rest) s_slow[wv][lane] = moved;
        __builtin_amdgcn_wave_barrier();
        n_slow = rest;
    };
    for (;;) {
        // ---- round: cells whose scan reached the end of the text, or whose end-cell diagonal passed the cut
        // (D[j + m - n][j] > cut proves the distance > cut: values never decrease along a diagonal), get their
        // level into the result buffer
        {
            bool fin = false;
            int lev = 0;
            if (active) {
                const int i_end = run ? j + (m - n) : m;  // the end cell's diagonal, or row m at j = n
                const Word M = i_end >= 64 ? ~(Word)0 : (((Word)1 << i_end) - 1);  // rows [0, i_end), 1 <= i_end <= 64
                const int d = j + __builtin_popcountll(VP & M) - __builtin_popcountll(VN & M);
                fin = !run || d > cut;
                lev = d > cut ? cut + 1 : d;
            }
            const unsigned long long fm = __ballot(fin);
            if (fm) {
                if (fin) {
                    const int r = n_res + __popcll(fm & below);
                    s_res[wv][0][r] = (uint32_t)p;
                    s_res[wv][1][r] = (uint32_t)(level_of(lev, S) + 1) * stride;
                    active = run = false;
                }
                __builtin_amdgcn_wave_barrier();
                n_res += __popcll(fm);
                if (n_res > 64) flush_res();  // (a batch flushes it; this only when batches ran out)
            }
        }
        // a text past 32 units: its next plane words move down whenever the scan reaches a multiple of 32 units
        // (blocks of LEVQ_STEPS steps start at multiples of LEVQ_STEPS, a divisor of 32)
        if (__any(run && j > 0 && (j & 31) == 0)) {
            if (run && j > 0 && (j & 31) == 0) {
#pragma unroll
                for (int b = 0; b < NP; ++b)
#pragma unroll
                    for (int h = 0; h + 1 < PW; ++h) T[PW * b + h] = T[PW * b + h + 1];
            }
        }
        const int n_act = __popcll(__ballot(active));
        // ---- batch: set up the next 64 cells when the queue is empty
        LEVQ_STAT(2, 1);
        if (q_count == 0 && bn < b_end && (64 - n_act >= LEVQ_ADOPT || n_act == 0)) {
#ifdef SPK_LEVQ_STATS
            const unsigned long long t_b = clock64();
            LEVQ_STAT(1, 1);
#endif
            // Order: (0) a full output buffer's device atomic (its return waits for everything in flight -- here
            // only the previous batch's loads and code adds), (1) the setup from the staged registers, (2) the
            // next prefetch loads, (3) LDS writes and fire-and-forget code adds: nothing after (2) waits on a load
            if (n_slow >= 64) flush_slow(64);
            const int32_t pc = p0;
            const int64_t left = n_items - bn * 64;
            const bool valid = lane < left && pc >= 0;
            bool to_slow = false, done = false, scan = false, a_pat = false;
            int level = 0, pre = 0, mm = 0, nn = 0, c = 0, s2 = 0;
            if (valid) {
                const RecMeta ma = {ska, sla, 0, sha, 0, sfa}, mb = {skb, slb, 0, shb, 0, sfb};
                const int la = sla, lb = slb;
                const int na = meta_cplen(ma), nb = meta_cplen(mb);
                s2 = na + nb;
                const bool planes = (sfa & CPF_PLANES) && (sfb & CPF_PLANES);  // 64-bit planes on both sides
                if (la < 0 || lb < 0) {
                    level = sc.null_level;
                    done = true;
                } else {
                    int eq = meta_equal(ma, mb);
                    if (eq < 0 && planes) {  // hash match without dictionary ids: the planes are the units
                        bool same = la == lb;
#pragma unroll
                        for (int b = 0; b < NP; ++b) same = same && sqa[b] == sqb[b];
                        eq = same ? 1 : 0;
                    }
                    if (eq == 1) {
                        level = lev_level_of(sc, 1, 0, s2);
                        done = true;
                    } else if (!planes) {
                        to_slow = true;
                    } else {
                        c = s_cut[s2];
                        int lev = -1;
                        if (la == 0 || lb == 0) {
                            lev = la + lb;
                        } else {
                            const int mn = la < lb ? la : lb;
                            Word d = 0, e = 0;
#pragma unroll
                            for (int b = 0; b < NP; ++b) {
                                d |= sqa[b] ^ sqb[b];
                                e |= (sqa[b] << (64 - la)) ^ (sqb[b] << (64 - lb));
                            }
                            pre = d ? __ffsll((unsigned long long)d) - 1 : 64;
                            if (pre > mn) pre = mn;
                            int suf = e ? __clzll((long long)e) : 64;
                            if (suf > mn - pre) suf = mn - pre;
                            const int ra = la - pre - suf, rb = lb - pre - suf;
                            if (ra == 0 || rb == 0) {
                                lev = ra + rb;
                            } else {
                                a_pat = ra >= rb;
                                mm = a_pat ? ra : rb;
                                nn = a_pat ? rb : ra;
                                if (mm - nn > c) lev = c + 1;  // the length gap alone exceeds the cut
                                else scan = true;
                            }
                        }
                        if (!scan) {
                            level = level_of(lev > c ? c + 1 : lev, s2);
                            done = true;
                        }
                    }
                }
            }
            // scan cells into the (empty) queue: the stripped planes, the longer remainder as the pattern
            const unsigned long long sm = __ballot(scan);
            if (scan) {
                const int r = __popcll(sm & below);
#pragma unroll
                for (int b = 0; b < NP; ++b) {
                    const Word pp = (a_pat ? sqa[b] : sqb[b]) >> pre;
                    const Word tt = (a_pat ? sqb[b] : sqa[b]) >> pre;
#pragma unroll
                    for (int h = 0; h < PW; ++h) {
                        s_q[wv][PW * b + h][r] = (uint32_t)(pp >> (32 * h));
                        s_q[wv][PW * NP + PW * b + h][r] = (uint32_t)(tt >> (32 * h));
                    }
                }
                s_q[wv][QP][r] = (uint32_t)pc;
                s_q[wv][QP + 1][r] = (uint32_t)mm | ((uint32_t)nn << 8) | ((uint32_t)c << 16) | ((uint32_t)s2 << 24);
            }
            q_head = 0;
            q_count = __popcll(sm);
            LEVQ_STAT(8, q_count);
            // cells this pass cannot scan into the output buffer
            const unsigned long long wm = __ballot(to_slow);
            if (wm) {
                if (to_slow) s_slow[wv][n_slow + __popcll(wm & below)] = pc;
                n_slow += __popcll(wm);
            }
            __builtin_amdgcn_wave_barrier();
            // the prefetch pipeline moves one batch on: rows of bn + 1, row ids of bn + 2, entries of bn + 3
            ++bn;
            stage(x1, y1);
            x1 = A.pl[pair_of(p2)];
            y1 = A.pr[pair_of(p2)];
            p0 = p1;
            p1 = p2;
            p2 = entry(bn + 2);
            // settled cells' and buffered code adds (fire-and-forget)
            if (done) code_add_atomic(A, pc, (uint32_t)(level + 1) * stride);
            if (n_res) flush_res();
            __builtin_amdgcn_wave_barrier();
#ifdef SPK_LEVQ_STATS
            LEVQ_STAT(9, clock64() - t_b);
#endif
        }
        // ---- round: idle lanes take queued cells
        if (q_count > 0) {
            const unsigned long long im = __ballot(!active);
            const int n_idle = __popcll(im);
            if (n_idle >= LEVQ_ADOPT || 64 - n_idle < LEVQ_ADOPT) {
                LEVQ_STAT(3, 1);
                const int r = __popcll(im & below);
                if (!active && r < q_count) {
                    const int e = q_head + r;
#pragma unroll
                    for (int b = 0; b < PW * NP; ++b) {
                        P[b] = s_q[wv][b][e];
                        T[b] = s_q[wv][PW * NP + b][e];
                    }
                    p = (int32_t)s_q[wv][QP][e];
                    const uint32_t pk = s_q[wv][QP + 1][e];
                    m = (int)(pk & 0xFF);
                    n = (int)((pk >> 8) & 0xFF);
                    cut = (int)((pk >> 16) & 0xFF);
                    S = (int)(pk >> 24);
                    VP = ~(Word)0;
                    VN = 0;
                    j = 0;
                    active = run = true;
                }
                const int taken = n_idle < q_count ? n_idle : q_count;
                q_head += taken;
                q_count -= taken;
            }
        }
        if (!__any(active)) {
            if (bn >= b_end && q_count == 0) break;
            continue;
        }
        // ---- LEVQ_STEPS scan steps of the lanes whose text has units left (a lane stops at j = n: its exec
        // bit drops, no branch).  The word width is a wave-uniform choice per block of steps: the full width only
        // when some scanning lane needs it in the block.  A pattern of more than H = 32 units needs it from
        // text unit J0 = (H - 1) - cut on (Ukkonen, as myers_plane_text_lazy): D[i][j] >= i - j, so rows > H
        // cannot hold a value <= cut before it, and until then a half-width step leaves rows H + 1 .. m at
        // D[H][j] + (i - H) (VP bits set, VN bits clear above row H) -- upper bounds that differ from the true
        // values only where both are > cut, so the cut tests and the clamped distance read the same.  The text's
        // plane words are read at bit j & 31 of T[PW b]; a lane's next words move down at multiples of 32 (in
        // the round, above).
        constexpr int H = 32;
        bool need_full = false;
        if (run && m > H) need_full = j + LEVQ_STEPS > (cut < H - 1 ? H - 1 - cut : 0);
        const bool wide = __any(need_full);
#ifdef SPK_LEVQ_STATS
        const unsigned long long t_s = clock64();
        LEVQ_STAT(wide ? 5 : 4, LEVQ_STEPS);
        LEVQ_STAT(7, __popcll(__ballot(run)));
#endif
        if (!wide) {
            typedef uint32_t Half;
            for (int s = 0; s < LEVQ_STEPS; ++s) {
                if (run) {
                    const uint32_t jj = (uint32_t)j & 31u;
                    Half eq = ~(Half)0;
#pragma unroll
                    for (int b = 0; b < NP; ++b) {
                        const uint32_t mb = (uint32_t)__builtin_amdgcn_sbfe((int)T[PW * b], jj, 1);
                        eq = eq_plane(eq, mb, P[PW * b]);
                    }
                    Half vp = (Half)VP, vn = (Half)VN;
                    const Half x = eq | vn;
                    const Half d0 = (((x & vp) + vp) ^ vp) | x;
                    const Half hp = (vn | ~(d0 | vp)) << 1 | (Half)1;
                    const Half hn = (d0 & vp) << 1;
                    vp = hn | ~(d0 | hp);
                    vn = hp & d0;
                    VP = (~(Word)0 << H) | (Word)vp;  // rows H + 1 .. m: D[H][j] + (i - H)
                    VN = (Word)vn;
                    ++j;
                    run = j < n;
                }
            }
        } else {
            for (int s = 0; s < LEVQ_STEPS; ++s) {
                if (run) {
                    const uint32_t jj = (uint32_t)j & 31u;
                    uint32_t e[PW];
#pragma unroll
                    for (int h = 0; h < PW; ++h) e[h] = ~0u;
#pragma unroll
                    for (int b = 0; b < NP; ++b) {
                        const uint32_t mb = (uint32_t)__builtin_amdgcn_sbfe((int)T[PW * b], jj, 1);
#pragma unroll
                        for (int h = 0; h < PW; ++h) e[h] = eq_plane(e[h], mb, P[PW * b + h]);
                    }
                    Word eq = 0;
#pragma unroll
                    for (int h = 0; h < PW; ++h) eq |= (Word)e[h] << (32 * h);
                    const Word x = eq | VN;
                    const Word d0 = (((x & VP) + VP) ^ VP) | x;
                    const Word hp = (VN | ~(d0 | VP)) << 1 | (Word)1;
                    const Word hn = (d0 & VP) << 1;
                    VP = hn | ~(d0 | hp);
                    VN = hp & d0;
                    ++j;
                    run = j < n;
                }
            }
        }
#ifdef SPK_LEVQ_STATS
        LEVQ_STAT(10, clock64() - t_s);
#endif
    }
#ifdef SPK_LEVQ_STATS
    LEVQ_STAT(11, clock64() - t_loop);
    LEVQ_STAT(0, 1);
    if (lane == 0)
        for (int i = 0; i < 12; ++i) atomicAdd(&g_levq[i], st_[i]);
#endif
    if (n_res) flush_res();
    if (n_slow >= 64) flush_slow(64);
    if (n_slow) flush_slow(n_slow);
}

// Global-memory pass over column k's slow list (length on the device; usually empty).  Cells with a
// string past SLOW_LIMIT units go on to the huge pass: their list (counter slow_count[2K + k]) takes
// column k's exact-list region, free once the exact pass ran and at least as long as the slow list.
template <bool SET>
__device__ __forceinline__ void gamma_slow_body(const GammaArgs &A, const ColSet &cs, int32_t *xlist, const int64_t *xinfo) {
    const int k = cs.k[blockIdx.y];
    const int64_t n = A.slow_count[k];
    const int32_t *items = A.slow + A.slow_off[k];
    int32_t *huge = xlist + xinfo[k];
    for (int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 64) {
        const int32_t p = items[i];
        int level = 0;
        const bool done = eval_column<M_SLOW, SET>(A, k, A.pl[p], A.pr[p], level) == ST_DONE;
        // several columns in one launch (the fused JW lists) can hold the same pair: their adds to its code race
        if (done && cs.n > 1) code_add_atomic(A, p, (uint32_t)(level + 1) * (uint32_t)A.stride[k]);
        else if (done) code_add(A, p, (uint32_t)(level + 1) * (uint32_t)A.stride[k]);
        wave_append(huge, A.slow_count + 2 * A.K + k, !done, p);
    }
}
__global__ __launch_bounds__(64) void k_gamma_slow(GammaArgs A, ColSet cs, int32_t *xlist, const int64_t *xinfo) {
    gamma_slow_body<false>(A, cs, xlist, xinfo);
}
__global__ __launch_bounds__(64) void k_gamma_slow_set(GammaArgs A, ColSet cs, int32_t *xlist, const int64_t *xinfo) {
    gamma_slow_body<true>(A, cs, xlist, xinfo);
}

// Huge pass: cells with a string longer than SLOW_LIMIT units, one lane per cell, DP rows and flag
// words in device scratch sized by the host to the longest string the column's program can meet.
template <bool SET>
__device__ __forceinline__ void gamma_huge_body(const GammaArgs &A, int k, const int32_t *items, int64_t n, Scratch &S) {
    S.slot = (int64_t)blockIdx.x * 64 + threadIdx.x;
    for (int64_t i = S.slot; i < n; i += S.n_slots) {
        const int32_t p = items[i];
        int level = 0;
        eval_column<M_HUGE, SET>(A, k, A.pl[p], A.pr[p], level, S);
        code_add(A, p, (uint32_t)(level + 1) * (uint32_t)A.stride[k]);
    }
}
__global__ __launch_bounds__(64) void k_gamma_huge(GammaArgs A, int k, const int32_t *items, int64_t n, Scratch S) {
    gamma_huge_body<false>(A, k, items, n, S);
}
__global__ __launch_bounds__(64) void k_gamma_huge_set(GammaArgs A, int k, const int32_t *items, int64_t n, Scratch S) {
    gamma_huge_body<true>(A, k, items, n, S);
}

// Slow list of a Levenshtein template column: cells whose rows are Latin-1 and at most
// PLANES2_MAX units (CPF_PLANES / CPF_PLANES2) are exact from 128-bit planes in registers
// (lev_rows_planes128) -- free-text columns such as cfg5's addresses land here; any other cell
// (non-Latin-1 or longer rows) runs the global-memory evaluation of k_gamma_slow.
template <bool P8>
__device__ int lev_cell128(const SimpleCol &sc, const ColDesc &c0, const ColDesc &c1, int32_t x, int32_t y,
                           int &level) {
    // One memory round trip: both rows' records, planes and upper planes are requested together (the upper
    // planes unconditionally -- from the lower planes' own row when the column has none -- and masked by the
    // records' flags afterwards), through global-address-space views.  Loading the upper planes only after the
    // records said a row has them took two round trips more per cell (item, pair rows, records, planes).
    const RecMeta ma = load_meta_global(c0.meta, x), mb = load_meta_global(c1.meta, y);
    uint64_t la[N_PLANES], lb[N_PLANES], ua[N_PLANES], ub[N_PLANES];
    {
        GU64 *qa = (GU64 *)(c0.planes + (int64_t)x * N_PLANES), *qb = (GU64 *)(c1.planes + (int64_t)y * N_PLANES);
        GU64 *ra = (GU64 *)((c0.planes_hi ? c0.planes_hi : c0.planes) + (int64_t)x * N_PLANES);
        GU64 *rb = (GU64 *)((c1.planes_hi ? c1.planes_hi : c1.planes) + (int64_t)y * N_PLANES);
#pragma unroll
        for (int i = 0; i < N_PLANES; ++i) {
            la[i] = qa[i];
            lb[i] = qb[i];
            ua[i] = ra[i];
            ub[i] = rb[i];
        }
    }
    if (ma.len16 < 0 || mb.len16 < 0) {
        level = sc.null_level;
        return ST_DONE;
    }
    constexpr uint32_t ANY = CPF_PLANES | CPF_PLANES2;
    if (!(ma.cpf & ANY) || !(mb.cpf & ANY)) return ST_NEEDS_SLOW;
    if (((ma.cpf & CPF_PLANES2) && !c0.planes_hi) || ((mb.cpf & CPF_PLANES2) && !c1.planes_hi)) return ST_NEEDS_SLOW;
    const uint64_t ka = (ma.cpf & CPF_PLANES2) ? ~0ull : 0ull, kb = (mb.cpf & CPF_PLANES2) ? ~0ull : 0ull;
    u128 pa[N_PLANES], pb[N_PLANES];
#pragma unroll
    for (int i = 0; i < N_PLANES; ++i) {
        pa[i] = ((u128)(ua[i] & ka) << 64) | la[i];
        pb[i] = ((u128)(ub[i] & kb) << 64) | lb[i];
    }
    int eq = meta_equal(ma, mb);
    if (eq < 0) {  // equal keys without dictionary ids: the planes are the units
        eq = ma.len16 == mb.len16 ? 1 : 0;
#pragma unroll
        for (int b = 0; b < N_PLANES; ++b) eq &= pa[b] == pb[b] ? 1 : 0;
    }
    const int na = meta_cplen(ma), nb = meta_cplen(mb);  // = len16: Latin-1 rows
    int lev = -1;
    for (int i = 0; i < sc.n_tests; ++i) {
        const int op = sc.op[i], cmp = sc.cmp[i];
        const double t = sc.t[i];
        int r;
        if (op == SPK_OP_STR_CMP) {
            r = ((eq == 1) == (cmp == SPK_CMP_EQ)) ? KT : KF;
        } else {
            const double den = (double)(na + nb) / 2.0;
            if (op == SPK_OP_LEVRATIO && den == 0.0) {
                r = KN;
            } else {
                if (lev < 0)
                    lev = eq == 1 ? 0 : lev_rows_planes128<P8>(pa, ma.len16, pb, mb.len16, simple_lev_cut(sc, na, nb), sc.np);
                r = op == SPK_OP_LEV ? cmpd((double)lev, t, cmp) : cmpd((double)lev / den, t, cmp);
            }
        }
        if (r == KT) {
            level = sc.level[i];
            return ST_DONE;
        }
    }
    level = sc.else_level;
    return ST_DONE;
}

// Cells without planes on both rows are handed on (rest list: column k's exact-list region, free
// once the exact pass ran, and counter slow_count[K + k]) to k_gamma_rest, so this kernel does not
// carry the general interpreter's registers (the 128-bit scan alone holds ~100).
template <bool P8>  // the column's scans read all 8 planes (SimpleCol.np == 8)
__global__ __launch_bounds__(X_THREADS) void k_gamma_slow_lev(GammaArgs A, int si, int32_t *xlist,
                                                              const int64_t *xinfo) {
    __shared__ SimpleCol s_sc;
    __shared__ ColDesc s_c0, s_c1;
    if (threadIdx.x == 0) {
        s_sc = A.simple[si];
        s_c0 = A.cols0[s_sc.col];
        s_c1 = A.cols1[s_sc.col];
    }
    __syncthreads();
    const int k = s_sc.k;
    const int64_t n = A.slow_count[k];
    const int32_t *items = A.slow + A.slow_off[k];
    int32_t *rest = xlist + xinfo[k];
    // (regrouping these cells by work bin, as k_gamma_exact_simple does for free-text columns,
    // measured no faster here: 2.43-2.47 ms per cfg5 call either way)
    // Software pipeline as the exact pass: the next cell's pair rows are in flight during this cell's scan, and
    // the list entry after that one a round earlier still (unconditional loads at clamped indices).
    const int64_t stride = (int64_t)gridDim.x * X_THREADS;
    int64_t i = (int64_t)blockIdx.x * X_THREADS + threadIdx.x;
    if (n <= 0) return;
    int32_t p = items[i < n ? i : n - 1];
    int32_t x = A.pl[p], y = A.pr[p];
    int32_t pn = items[i + stride < n ? i + stride : n - 1];
    for (; i < n; i += stride) {
        const int32_t x2 = A.pl[pn], y2 = A.pr[pn];
        const int64_t i3 = i + 2 * stride;
        const int32_t pn3 = items[i3 < n ? i3 : n - 1];
        int level = 0;
        const bool done = lev_cell128<P8>(s_sc, s_c0, s_c1, x, y, level) == ST_DONE;
        if (done) code_add(A, p, (uint32_t)(level + 1) * (uint32_t)A.stride[k]);
        wave_append(rest, A.slow_count + A.K + k, !done, p);
        p = pn;
        x = x2;
        y = y2;
        pn = pn3;
    }
}

// The rest list of k_gamma_slow_lev through the global-memory evaluation; cells past SLOW_LIMIT
// units go to the huge list, in column k's slow-list region (free once k_gamma_slow_lev ran).
__global__ __launch_bounds__(64) void k_gamma_rest(GammaArgs A, int k, const int32_t *xlist, const int64_t *xinfo) {
    const int64_t n = A.slow_count[A.K + k];
    const int32_t *items = xlist + xinfo[k];
    int32_t *huge = A.slow + A.slow_off[k];
    for (int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 64) {
        const int32_t p = items[i];
        int level = 0;
        const bool done = eval_column<M_SLOW>(A, k, A.pl[p], A.pr[p], level) == ST_DONE;
        if (done) code_add(A, p, (uint32_t)(level + 1) * (uint32_t)A.stride[k]);
        wave_append(huge, A.slow_count + 2 * A.K + k, !done, p);
    }
}

// ---- launch logic (host) -----------------------------------------------------------------------------
// Device scratch of a huge pass over `cells` cells whose strings have at most `units` UTF-16 units: a
// slot per lane (JW: two flag-word arrays; Levenshtein: code points + one DP row; jaccard_sim: two
// presence bitmaps over the unit values), lanes = one per cell, at most ~1 GiB of slots, at least one wave.
int huge_scratch(int64_t units, int64_t cells, DevBuf<uint8_t> &buf, Scratch &S) {
    SPK_REQUIRE(units < INT32_MAX / 2, SPK_E_LIMIT, "a compared string is longer than 2^30 UTF-16 units");
    S.units = (int32_t)units;
    S.words = (int32_t)((units + 63) / 64);
    const int64_t slot_bytes = std::max<int64_t>({16 * (int64_t)S.words, 4 * (2 * units + 1), 16 * (int64_t)JACCARD_WORDS});
    const int64_t budget = std::max<int64_t>(64, ((int64_t)1 << 30) / slot_bytes / 64 * 64);
    S.n_slots = std::min<int64_t>(budget, (cells + 63) / 64 * 64);
    SPK_TRY(buf.alloc((size_t)(S.n_slots * slot_bytes)));
    S.base = buf.p;
    return SPK_OK;
}

int enqueue_slow(spk_ctx *ctx, Slot &S, int k, const ColSet *jk) {
    const GammaCols &C = *ctx->gcols;
    GammaPlan &G = *S.gplan;
    GammaArgs &A = G.A;
    if (jk) {
        k_gamma_slow<<<dim3((unsigned)(4 * ctx->n_cu), (unsigned)jk->n), 64, 0, S.stream>>>(A, *jk, S.xlist.p,
                                                                                              S.xinfo.p);
    } else {
        const int si = C.simple_of[k];
        const bool lev = si >= 0 && C.simple[si].cls == SC_LEV;
        const ColSet one_k{1, {k, 0, 0, 0}};
        if (lev) {
            // (a lane-refill form of this pass over 128-bit planes lost 0.5 ms per cfg5 γ pass)
            constexpr int SLOWLEV_WG_PER_CU = 8;  // the 128-bit scan holds 3 waves per SIMD: 3 workgroups per CU at once
            const int64_t g_sl = std::max<int64_t>(1, std::min<int64_t>(G.g_exact, (int64_t)SLOWLEV_WG_PER_CU * ctx->n_cu));
            if (C.simple[si].np >= N_PLANES)
                k_gamma_slow_lev<true><<<(unsigned)g_sl, X_THREADS, 0, S.stream>>>(A, si, S.xlist.p, S.xinfo.p);
            else
                k_gamma_slow_lev<false><<<(unsigned)g_sl, X_THREADS, 0, S.stream>>>(A, si, S.xlist.p, S.xinfo.p);
            k_gamma_rest<<<(unsigned)(4 * ctx->n_cu), 64, 0, S.stream>>>(A, k, S.xlist.p, S.xinfo.p);
        } else {
            k_gamma_slow<<<(unsigned)(4 * ctx->n_cu), 64, 0, S.stream>>>(A, one_k, S.xlist.p, S.xinfo.p);
        }
    }
    SPK_HIP(hipGetLastError());
    return SPK_OK;
}

int enqueue_phase(spk_ctx *ctx, Slot &S, int64_t cap, bool skip) {
    const GammaCols &C = *ctx->gcols;
    GammaPlan &G = *S.gplan;
    GammaArgs &A = G.A;
    const int K = C.K;
    G.slow_skipped.assign((size_t)K, 0);
    auto quiet = [&](int k) {
        return skip && (ctx->slow_force_skip ||
                        (ctx->slow_seen_valid && k < (int)ctx->slow_seen.size() && !ctx->slow_seen[k]));
    };
    SPK_TRY(S.xlist.alloc((size_t)(2 * cap)));
    A.slow = S.xlist.p + cap;
    A.slow_off = S.xinfo.p;
    S.xcap = cap;
    if (A.P <= 0) {
        SPK_HIP(hipMemsetAsync(S.xinfo.p, 0, (size_t)C.n_info * 8, S.stream));
        return SPK_OK;
    }
    k_prefix<<<(unsigned)K, PFX_THREADS, 0, S.stream>>>(
        S.region_count.p, K, G.n_regions, cap, S.xpref.p, S.xinfo.p,
        reinterpret_cast<unsigned long long *>(S.xinfo.p + C.n_info + C.n_cnt + 1));
    const std::vector<SimpleCol> &simple = C.simple;
    // Jaro-Winkler template columns: compact every list, then one exact launch over all of them
    // JW exact launches: a JW cell is one short latency-bound evaluation, and the kernel holds 3 waves per
    // SIMD, so a grid of 8 workgroups per CU ran in rounds of dispatch latency; JW_WG_PER_CU per column
    // keeps it near one resident round with the grid-stride loop's prefetch
    constexpr int JW_WG_PER_CU = 8;
    const int64_t g_jw = std::max<int64_t>(1, std::min<int64_t>(G.g_exact, (int64_t)JW_WG_PER_CU * ctx->n_cu));
    ExactCols jw{};
    jw.g = (int)g_jw;
    ColSet jk{};
    for (int k = 0; k < K; ++k) {
        if (!C.may_exact[k] || C.simple_of[k] < 0) continue;
        const SimpleCol &sc = simple[C.simple_of[k]];
        if (sc.cls != SC_JW || sc.kind != SK_STR || jw.n == 4) continue;
        jk.k[jk.n++] = k;
        jw.k[jw.n] = sc.k;
        jw.col[jw.n] = sc.col;
        jw.si[jw.n++] = C.simple_of[k];
    }
    // One compaction launch for the JW lists and the other plain-compacted lists (up to four columns): the
    // launch is one workgroup per region and column, and a short list's workgroups cost dispatch rounds alone
    // (cfg2: the JW lists' launch took as long as the email list's, 15 us each)
    ColSet pre = jk;
    for (int k = 0; k < K && pre.n < 4; ++k) {
        if (!C.may_exact[k]) continue;
        const int si = C.simple_of[k];
        bool in_jw = false;
        for (int c = 0; c < jw.n; ++c) in_jw = in_jw || jw.si[c] == si;
        if (in_jw || (si >= 0 && simple[si].cls == SC_LEV && C.bag[k])) continue;
        pre.k[pre.n++] = k;
    }
    auto precompacted = [&](int k) {
        for (int c = 0; c < pre.n; ++c)
            if (pre.k[c] == k) return true;
        return false;
    };
    if (pre.n)
        k_compact<<<dim3((unsigned)G.n_regions, (unsigned)pre.n), 256, 0, S.stream>>>(A, pre, S.xpref.p,
                                                                                        S.xlist.p, S.xinfo.p);
    // (running this launch on a second stream beside the Levenshtein pass measured no faster:
    // 1.198-1.205 ms per cfg2 pass either way)
    for (int c = 0; c < K; ++c)
        if (c < (int)S.xev_used.size()) S.xev_used[c] = 0;
    if (jw.n) {
        SPK_TRY(ctx->xbegin(S, jk.k[0]));
        k_gamma_exact_simple<X_JW><<<(unsigned)(g_jw * jw.n), X_THREADS, 0, S.stream>>>(A, jw, S.xlist.p,
                                                                                                S.xinfo.p);
        SPK_TRY(ctx->xend(S, jk.k[0]));
        bool all_quiet = true;
        for (int c = 0; c < jk.n; ++c) all_quiet = all_quiet && quiet(jk.k[c]);
        if (all_quiet) {
            for (int c = 0; c < jk.n; ++c) G.slow_skipped[jk.k[c]] = 1;
        } else {
            SPK_TRY(enqueue_slow(ctx, S, -1, &jk));
        }
    }
    for (int k = 0; k < K; ++k) {
        if (!C.may_exact[k]) continue;
        const int si = C.simple_of[k];
        const bool lev = si >= 0 && simple[si].cls == SC_LEV;
        bool fused = false;
        for (int c = 0; c < jw.n; ++c) fused = fused || jw.si[c] == si;
        if (fused) continue;
        const ColSet one_k{1, {k, 0, 0, 0}};
        const bool refill = lev && (ctx->lev_kernel == 1 || (ctx->lev_kernel == 2 && C.free_text[k]));
        if (lev && C.bag[k])
            k_compact_lev<<<(unsigned)G.n_regions, CL_THREADS, 0, S.stream>>>(A, k, si, S.xpref.p, S.xlist.p,
                                                                                S.xinfo.p);
        else if (!precompacted(k))
            k_compact<<<(unsigned)G.n_regions, 256, 0, S.stream>>>(A, one_k, S.xpref.p, S.xlist.p, S.xinfo.p);
        if (refill) {
            // one resident round (LEVQ_WAVES per SIMD, 3 for NP = 8): every wave owns a contiguous range of the list
            const int64_t wg_cu = simple[si].np >= 8 ? 3 : LEVQ_WG_PER_CU;
            const int64_t g_lev = std::max<int64_t>(1, std::min<int64_t>(G.g_exact, wg_cu * ctx->n_cu));
            SPK_TRY(ctx->xbegin(S, k));
            switch (simple[si].np) {
                case 5: k_lev_refill<5><<<(unsigned)g_lev, X_THREADS, 0, S.stream>>>(A, si, S.xlist.p, S.xinfo.p); break;
                case 6: k_lev_refill<6><<<(unsigned)g_lev, X_THREADS, 0, S.stream>>>(A, si, S.xlist.p, S.xinfo.p); break;
                case 7: k_lev_refill<7><<<(unsigned)g_lev, X_THREADS, 0, S.stream>>>(A, si, S.xlist.p, S.xinfo.p); break;
                default: k_lev_refill<8><<<(unsigned)g_lev, X_THREADS, 0, S.stream>>>(A, si, S.xlist.p, S.xinfo.p); break;
            }
            SPK_TRY(ctx->xend(S, k));
            if (quiet(k)) G.slow_skipped[k] = 1;
            else SPK_TRY(enqueue_slow(ctx, S, k, nullptr));
        } else if (lev) {
            ExactCols one{};
            one.n = 1;
            // one resident round: the grid-stride loop gives every block a fixed share of the list, so a
            // grid larger than what fits at once (LEV_WAVES per SIMD) runs a second, partly empty round
            constexpr int LEV_WG_PER_CU = 8;
            const int64_t g_lev = std::max<int64_t>(1, std::min<int64_t>(G.g_exact, (int64_t)LEV_WG_PER_CU * ctx->n_cu));
            one.g = (int)g_lev;
            one.si[0] = si;
            one.k[0] = simple[si].k;
            one.col[0] = simple[si].col;
            SPK_TRY(ctx->xbegin(S, k));
            k_gamma_exact_simple<X_LEV><<<(unsigned)g_lev, X_THREADS, 0, S.stream>>>(A, one, S.xlist.p,
                                                                                      S.xinfo.p);
            SPK_TRY(ctx->xend(S, k));
            if (quiet(k)) G.slow_skipped[k] = 1;
            else SPK_TRY(enqueue_slow(ctx, S, k, nullptr));
        } else if (si >= 0 && simple[si].kind == SK_STR) {
            ExactCols one{};
            one.n = 1;
            one.g = (int)G.g_exact;
            one.si[0] = si;
            one.k[0] = simple[si].k;
            one.col[0] = simple[si].col;
            k_gamma_exact_simple<X_GENERIC><<<(unsigned)G.g_exact, X_THREADS, 0, S.stream>>>(A, one, S.xlist.p,
                                                                                           S.xinfo.p);
            if (quiet(k)) G.slow_skipped[k] = 1;
            else SPK_TRY(enqueue_slow(ctx, S, k, nullptr));
        } else {
            // an interpreter column: the instantiations with jaccard_sim / cosine_distance only where it names them
            if (C.setsim[k]) {
                k_gamma_exact_set<<<(unsigned)G.g_exact, X_THREADS, 0, S.stream>>>(A, k, S.xlist.p, S.xinfo.p);
                k_gamma_slow_set<<<(unsigned)(4 * ctx->n_cu), 64, 0, S.stream>>>(A, one_k, S.xlist.p, S.xinfo.p);
            } else {
                k_gamma_exact<<<(unsigned)G.g_exact, X_THREADS, 0, S.stream>>>(A, k, S.xlist.p, S.xinfo.p);
                k_gamma_slow<<<(unsigned)(4 * ctx->n_cu), 64, 0, S.stream>>>(A, one_k, S.xlist.p, S.xinfo.p);
            }
        }
    }
    SPK_HIP(hipGetLastError());
    return SPK_OK;
}

// Cells with a string longer than SLOW_LIMIT units (none in the benchmark configs).  Column k's huge list starts
// at its list offset xinfo[k] (h_info holds it) of the slow-list or the exact-list region (GammaCols.huge_in_slow).
int run_huge(spk_ctx *ctx, Slot &S, const unsigned int *n_huge) {
    const GammaCols &C = *ctx->gcols;
    const GammaPlan &G = *S.gplan;
    int64_t max_huge = 0;
    for (int k = 0; k < C.K; ++k) max_huge = std::max<int64_t>(max_huge, n_huge[k]);
    Scratch Sc;
    DevBuf<uint8_t> scratch;
    SPK_TRY(huge_scratch(C.max_units, max_huge, scratch, Sc));
    for (int k = 0; k < C.K; ++k) {
        if (!n_huge[k]) continue;
        const int32_t *items = (C.huge_in_slow[k] ? G.A.slow : S.xlist.p) + S.h_info.p[k];
        if (C.setsim[k]) k_gamma_huge_set<<<(unsigned)(Sc.n_slots / 64), 64, 0, S.stream>>>(G.A, k, items, n_huge[k], Sc);
        else k_gamma_huge<<<(unsigned)(Sc.n_slots / 64), 64, 0, S.stream>>>(G.A, k, items, n_huge[k], Sc);
        SPK_HIP(hipGetLastError());
    }
    SPK_HIP(hipStreamSynchronize(S.stream));  // the scratch lives until here
    return SPK_OK;
}

#ifdef SPK_LEVQ_STATS
extern "C" int spk_debug_levq_stats(uint64_t *out, int reset) {
    SPK_HIP(hipDeviceSynchronize());
    SPK_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_levq), sizeof(uint64_t) * 16));
    if (reset) {
        static const unsigned long long zero[16] = {};
        SPK_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_levq), zero, sizeof(zero)));
    }
    return SPK_OK;
}
#endif

}  // namespace spk
