// Internal definitions shared by the libsplink_hip.so translation units (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../../include/splink_hip.h"

namespace spk {

// ---- error plumbing -------------------------------------------------------------------
void set_error(const std::string &msg);

#define SPK_HIP(expr)                                                                         \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess) {                                                               \
            ::spk::set_error(std::string(#expr) + ": " + hipGetErrorString(_e));              \
            return _e == hipErrorOutOfMemory ? SPK_E_OOM : SPK_E_HIP;                         \
        }                                                                                     \
    } while (0)

#define SPK_REQUIRE(cond, code, msg)                                                          \
    do {                                                                                      \
        if (!(cond)) {                                                                        \
            ::spk::set_error(msg);                                                            \
            return code;                                                                      \
        }                                                                                     \
    } while (0)

#define SPK_TRY(expr)                                                                         \
    do {                                                                                      \
        int _r = (expr);                                                                      \
        if (_r != SPK_OK) return _r;                                                          \
    } while (0)

// ---- device column layout ---------------------------------------------------------------
// String columns keep the UTF-16 code units of row i at a 4-unit (8-byte) aligned start derived
// from its UTF-8 byte offset, (off8[i] + 3i + 3) & ~3: UTF-16 never needs more units than UTF-8
// has bytes, so the starts are monotone, rows never overlap and no scan is needed on upload.
// Each row also has a 32-byte metadata record (two 16-byte loads) that holds everything the
// comparison filter needs -- NULL flag, lengths, equality key, sketch and the first four units --
// so most (pair, column) cells are decided without touching the units at all.
enum ColKind : int32_t { COL_NONE = 0, COL_STR = 1, COL_NUM = 2 };

struct alignas(16) RecMeta {
    uint32_t key;     // dictionary id of the value (CPF_ID: equal iff the strings are) or a 32-bit
                      // FNV-1a fold of the units (unequal keys prove unequal strings)
    int32_t len16;    // UTF-16 length, -1 = NULL
    uint64_t sketch;  // unit sketch (sketch_bucket / sketch_add)
    uint64_t head;    // units 0..3, zero beyond len16
    uint32_t off4;    // first UTF-16 unit of the row / 4 (rows start 8-byte aligned)
    uint32_t cpf;     // bits 0..23: code-point length; bit 24: bit-planes valid (<= 64 units, all < 256);
                      // bit 25: `key` is an exact dictionary id; bit 26: two-word bit-planes valid
                      // (65..128 units, all < 256: units 0..63 in planes, 64..127 in planes_hi)
};
static_assert(sizeof(RecMeta) == 32, "RecMeta layout");
constexpr uint32_t CPF_PLANES = 1u << 24;
constexpr uint32_t CPF_ID = 1u << 25;
constexpr uint32_t CPF_PLANES2 = 1u << 26;
constexpr int PLANES2_MAX = 128;  // longest row with two-word planes
__host__ __device__ inline int32_t meta_cplen(const RecMeta &m) { return (int32_t)(m.cpf & 0xFFFFFFu); }
__host__ __device__ inline int64_t meta_off(const RecMeta &m) { return (int64_t)m.off4 * 4; }

// Bit-planes of a row whose units are all < 256 and that has <= 64 units: plane b (0..7) holds
// bit b of unit i at bit i.  The Levenshtein / Jaro-Winkler match masks of a character c are then
// AND_b (bit b of c ? plane_b : ~plane_b), eight register ops instead of a scan of the string.
constexpr int N_PLANES = 8;

// Unit sketch: 32 buckets of saturating 2-bit unit counts (0, 1, 2, >=3) held as two bit-planes,
// bits 0..31 the low count bit and bits 32..63 the high count bit of each bucket.  ASCII letters
// get a bucket each (case folded), digits three, other ASCII three; other units are hashed.
// Merging units into a bucket only raises the per-bucket minima, so the multiset-intersection
// bound derived from two sketches (sketch_inter_ub) holds for any bucket map.
__host__ __device__ inline uint32_t sketch_bucket(uint32_t u) {
    if (u < 128u) {
        if (u >= 'a' && u <= 'z') return u - 'a';
        if (u >= 'A' && u <= 'Z') return u - 'A';
        if (u >= '0' && u <= '9') return 26u + (u - '0') % 3u;
        return 29u + u % 3u;
    }
    return ((u * 2654435761u) >> 16) & 31u;
}

__host__ __device__ inline void sketch_add(uint64_t &sk, uint32_t unit) {
    const uint32_t b = sketch_bucket(unit);
    const uint64_t lo = 1ull << b, hi = 1ull << (32 + b);
    if ((sk & lo) && (sk & hi)) return;  // saturated at 3
    if (sk & lo) sk = (sk & ~lo) | hi;   // 1 -> 2
    else sk |= lo;                       // 0 -> 1, 2 -> 3
}

// Positional sketch of a row that a template Levenshtein comparison reads (k_pos_rows, spk_ctx.hip; the filter's
// bound is in spk_filter.hip): the row's n code points split into the halves [0, ceil(n/2)) and [ceil(n/2), n),
// each with 30 buckets of saturating 2-bit counts as two bit-planes -- a bucket per ASCII letter (case folded), two
// for the digits, two for every other unit.  The 16-byte row, as one 128-bit value:
//   length (8 bits) | half-1 low plane << 8 | half-1 high plane << 38 | half-2 low plane << 68 | half-2 high << 98
// with length 255 = NULL and 254 = no sketch (254 code points or more, or a surrogate pair: its units are not its
// code points), which leaves the cell to the exact pass.
constexpr int POS_BUCKETS = 30;
constexpr uint32_t POS_MASK = (1u << POS_BUCKETS) - 1u;
constexpr uint32_t POS_NULL = 255u, POS_NONE = 254u;
__host__ __device__ inline uint32_t pos_bucket(uint32_t u) {
    if (u >= 'a' && u <= 'z') return u - 'a';
    if (u >= 'A' && u <= 'Z') return u - 'A';
    if (u >= '0' && u <= '9') return 26u + (u & 1u);
    return 28u + ((u >> 1) & 1u);
}

struct ColDesc {
    int32_t kind;
    int32_t pad;
    const uint16_t *units;   // COL_STR
    const RecMeta *meta;     // COL_STR
    const uint64_t *planes;  // COL_STR, [n][N_PLANES]
    const uint64_t *planes_hi;  // COL_STR, [n][N_PLANES] units 64..127 (CPF_PLANES2 rows), or null
    const uint4 *bag;        // COL_STR: [n][2] character-bag rows (k_bag_rows), or null (not built)
    const uint4 *pos;        // COL_STR: [n] positional sketch rows (k_pos_rows), or null (not built)
    const double *val;       // COL_NUM
    const uint8_t *valid;   // COL_NUM
};

template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    int alloc(size_t count) {
        if (count <= n && p) return SPK_OK;
        release();
        if (count == 0) return SPK_OK;
        hipError_t e = hipMalloc(&p, count * sizeof(T));
        if (e != hipSuccess) {
            p = nullptr;
            set_error(std::string("hipMalloc failed: ") + hipGetErrorString(e));
            return e == hipErrorOutOfMemory ? SPK_E_OOM : SPK_E_HIP;
        }
        n = count;
        return SPK_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    ~DevBuf() { release(); }
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), n(o.n) {
        o.p = nullptr;
        o.n = 0;
    }
    DevBuf &operator=(DevBuf &&o) noexcept {  // frees what this buffer held
        if (this != &o) {
            release();
            std::swap(p, o.p);
            std::swap(n, o.n);
        }
        return *this;
    }
};

// A pinned host buffer that only grows; growing drops what it held.  Freed with its owner: a context is deleted with
// its device set (spk_ctx_destroy).
template <typename T>
struct PinnedBuf {
    T *p = nullptr;
    size_t n = 0;
    int grow(size_t count) {
        if (count <= n) return SPK_OK;
        release();
        if (hipHostMalloc(reinterpret_cast<void **>(&p), count * sizeof(T), hipHostMallocDefault) != hipSuccess) {
            p = nullptr;
            set_error("hipHostMalloc failed");
            return SPK_E_OOM;
        }
        n = count;
        return SPK_OK;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        n = 0;
    }
    ~PinnedBuf() { release(); }
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf &) = delete;
    PinnedBuf &operator=(const PinnedBuf &) = delete;
};

struct Column {
    ColKind kind = COL_NONE;
    DevBuf<uint16_t> units;
    int64_t units_len = 0;  // units written by the last decode (zeroed first); the buffer may be larger (reused)
    DevBuf<RecMeta> meta;
    DevBuf<uint64_t> planes;
    DevBuf<uint64_t> planes_hi;  // allocated only when some row has more than 64 UTF-8 bytes
    DevBuf<uint4> bag;           // 32-byte character-bag row per row (k_bag_rows; built when a Levenshtein
                                 // comparison reads the column)
    DevBuf<uint4> pos;           // 16-byte positional sketch per row (k_pos_rows; built when a template Levenshtein
                                 // comparison reads a column without free-text rows)
    DevBuf<double> val;
    DevBuf<uint8_t> valid;
    bool has_ids = false;  // COL_STR: RecMeta.key is a dictionary id
    int64_t max_bytes = 0; // COL_STR: longest row in UTF-8 bytes (>= its UTF-16 units)
    uint64_t src[2] = {0, 0};  // spk_table_add_raw_utf8: serials of the raw columns of the l / r side (0: other)
    bool has_empty = false;    // some non-NULL row is the empty string
    int64_t n_ids = -1;        // spk_table_add_raw_utf8: distinct non-NULL values (ids are dense in [0, n_ids))
    // OR / AND of the units of every row that has bit-planes (bits 0..7), set by launch_unit_bits
    bool unit_bits = false;
    uint32_t unit_or = 0, unit_and = 0xFFu;
};

// A blocking-key term as spk_key_build saw it, by raw-column serial: the comparison filter skips a
// string column for the pairs of a rule whose key includes `l.c = r.c` on that column's own raw
// columns (the strings are then equal and non-NULL; see spk_gammas).
struct KeyTerm {
    uint64_t src_l = 0, src_r = 0;
    bool plain = false;  // no substr on either side
};

// An input column as handed over (Arrow buffers), kept on the device in input row order: the source
// of blocking keys, dictionary ids and (through a table's row permutation) comparison columns.
enum RawKind : int32_t { RAW_UTF8 = 1, RAW_I64 = 2 };
struct RawCol {
    RawKind kind = RAW_UTF8;
    uint64_t serial = 0;     // ctx-wide upload counter (a replaced raw column gets a new one)
    bool has_empty = false;  // RAW_UTF8: some non-NULL value is the empty string
    int64_t n = 0;
    int64_t max_len = 0;     // longest value in bytes (UTF-8)
    DevBuf<int64_t> off;     // RAW_UTF8: n + 1 byte offsets
    DevBuf<uint8_t> bytes;   // RAW_UTF8
    DevBuf<int64_t> i64;     // RAW_I64: values (compared as 8-byte patterns)
    DevBuf<uint8_t> valid;   // 1 = non-NULL
    bool released = false;   // spk_raw_release: buffers freed, serial kept
};

struct Table {
    int64_t n = -1;
    DevBuf<int32_t> perm;    // row i of the table is input row perm[i] (spk_cluster); empty = identity
    std::vector<Column *> cols;
    DevBuf<ColDesc> d_desc;
    bool desc_dirty = true;
    uint64_t version = 0;  // bumped (ctx-wide counter) whenever the table or one of its columns is replaced
    DevBuf<int64_t> rank;
    int64_t null_div = 0;  // rank layout for NULL unique ids (spk_table_set_rank_null), 0 = none
    std::vector<DevBuf<int64_t> *> key[2];  // [which][rule]
    ~Table();
};

// Blocking rule r >= 1 as its own row order ("view"): the rows with a non-NULL key r sorted by
// (key r, rank), so a block of rule r is contiguous in it.  Pairs of rule r also carry their view
// positions (spk_ctx::pvl / pvr), and the comparison filter reads a copy of the row image laid out
// in view order: the pairs of a later rule then touch a block's rows in a few cache lines, as the
// first rule's pairs do in the table (clustered by rule 0) itself.
constexpr int MAX_VIEWS = 2;  // rules 1 .. MAX_VIEWS - 1 get views (one: registers of the filter)
struct RuleView {
    DevBuf<int32_t> rowsL, rowsR;  // view position -> table row (l side; r side unless tri)
    int64_t nL = 0, nR = 0;
    bool tri = true;               // symmetric self-join: both sides index rowsL
    int64_t pair_lo = 0, pair_hi = 0;  // this rule's pair ordinals (local shard)
};

// First pair ordinal that carries view positions, given the first ordinal of every rule and the pair count:
// rule 1's first pair, or none when there is one rule (MAX_VIEWS = 2: only rule 1 has a view).
inline int64_t view_pair_base(const std::vector<int64_t> &rule_base, int64_t n_pairs) {
    return rule_base.size() > 1 ? rule_base[1] : n_pairs;
}

// The survivors of the last spk_select (spk_select.hip), in ascending pair ordinal.  It carries its own copy of
// the pattern space and its own mp-per-pattern table, so reading it back depends on nothing a later call rewrites;
// the three counters say which pairs and codes it was taken from (spk_select_copy refuses it once they moved on).
struct Selection {
    bool valid = false;
    int64_t n = 0;
    DevBuf<int64_t> ord;     // pair ordinal
    DevBuf<int32_t> l, r;    // the pair's rows (has_rows)
    DevBuf<uint32_t> code;   // its packed comparison code
    DevBuf<double> mpat;     // mp per pattern under spk_select's parameters (has_mp)
    bool has_rows = false, has_mp = false;
    // spk_select_tf*: the survivors' tf_adjusted_match_prob and their n_tf adjustments [n x n_tf] under that call's
    // tables (which are gone when it returns)
    bool has_tf = false;
    int n_tf = 0;
    DevBuf<double> tf_mp, adj;
    int K = 0;
    std::vector<int32_t> n_levels;
    std::vector<int64_t> stride;
    uint64_t pairs_epoch = 0, gamma_seq = 0, fix_seq = 0;
    double ms = -1.0;        // device milliseconds of its kernels (timing on), -1 = none
    bool current(const spk_ctx *ctx) const;  // taken from the context's present pairs and codes
    void clear() { *this = Selection(); }
};

// The labels of the last spk_components* (spk_components.hip): label[v] = the smallest node id of v's component, by
// node id (input position).  Built in a local and moved into the context, so a failing call leaves none; once built
// it needs neither the selection nor the codes nor the pairs, only that the tables (whose rows the ids name) stay.
struct Components {
    bool valid = false;
    int64_t n_nodes = 0, n_edges = 0, n_clusters = 0;
    int rounds = 0;
    DevBuf<uint32_t> label;  // [n_nodes]
    double ms = -1.0;        // device milliseconds of its kernels (timing on), -1 = none
    bool merged = false;     // spk_components_merge hooked other graphs' labels in: n_edges is still this graph's own
    void clear() { *this = Components(); }
};

// The labels of the last spk_components_sweep* (spk_components.hip): level k's labels are those of the graph whose edges
// are the selection's survivors (or the host edges) with score > thresholds[k].  A value of its own, independent of
// `Components`: built in a local and moved into the context, so a failing call leaves none.  It keeps the edges
// bucketed by level (8 bytes per edge), so spk_cluster_metrics can run later without the selection; the metrics of
// one level at a time live in it too (recomputed per call, freed with it).
// The bridges and cores of one level of the sweep (spk_bridges.hip), by node id.  A value of its own inside the sweep
// it describes: built in a local and moved in at the end of spk_cluster_bridges, so a failing call leaves none; gone
// with the sweep.  Nothing in it is read or written by the metrics, and it reads none of theirs.
struct ClusterBridges {
    int level = -1;  // -1: none
    int64_t n_nodes = 0, n_bridges = 0, n_cores = 0, largest_core = 0, depth = 0;
    int rounds = 0;            // forest rounds, the last quiet one included
    DevBuf<uint32_t> u, v, side_u, side_v;  // [n_bridges], ascending by (u, v)
    DevBuf<uint32_t> core;     // [n_nodes]
    double ms = -1.0;          // device milliseconds of its kernels (timing on), -1 = none
    void clear() { *this = ClusterBridges(); }
};

struct ComponentSweep {
    bool valid = false;
    int levels = 0;
    int64_t n_nodes = 0;
    std::vector<int64_t> off;         // [levels + 1] start of each level's range in eu / ev, every one a multiple of 4
    std::vector<int64_t> cnt;         // [levels] edges of the level; [off[k] + cnt[k], off[k + 1]) is (0, 0) padding
    std::vector<int64_t> n_edges;     // [levels] cumulative: edges with score > thresholds[k]
    std::vector<int64_t> n_clusters;  // [levels]
    std::vector<int> rounds;          // [levels]
    DevBuf<uint32_t> label;           // [levels x n_nodes], level-major; offsets into it are size_t
    DevBuf<uint32_t> eu, ev;          // the edges, bucketed by level
    double ms = -1.0;                 // device milliseconds of its kernels (timing on), -1 = none
    // spk_components_sweep_merge ran on a level: its labels are the union's, eu / ev still one shard's, so the degrees
    // would be partial and spk_cluster_metrics refuses
    bool merged = false;
    // spk_cluster_metrics: the level they describe (-1: none), by node id
    int m_level = -1;
    double m_ms = -1.0;
    DevBuf<uint32_t> degree, size, max_degree;
    DevBuf<unsigned long long> degree_sum;
    ClusterBridges bridges;  // spk_cluster_bridges: the level they describe is bridges.level
    void clear() { *this = ComponentSweep(); }
};

struct GammaCols;  // spk_gamma.h: a call's column decisions
struct GammaPlan;  // spk_gamma.h: one window's plan
enum Kern { K_BLOCK = 0, K_GAMMA = 1, K_EMHIST = 2, K_EMFIN = 3, K_SCORE = 4, K_COUNT = 5 };

}  // namespace spk

struct spk_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t own_stream = nullptr;
    spk::Table table[2];
    int link_type = SPK_LINK_DEDUPE;

    // candidate pairs (row indices into table 0 / table side_r)
    spk::DevBuf<int32_t> pl, pr;
    int64_t n_pairs = 0;
    bool pairs_valid = false;
    uint64_t pairs_epoch = 0;          // bumped whenever the pair set is replaced
    std::vector<spk::KeyTerm> rule_terms[32];   // spk_key_build terms per rule (cleared by spk_table_set_key)
    std::vector<std::vector<spk::KeyTerm>> pair_terms;  // the terms of each rule of the current pair set
    std::vector<int64_t> pair_rule_lo, pair_rule_hi;   // local pair ordinals of each rule (spk_block)
    uint64_t raw_serial = 0;
    spk::RuleView views[spk::MAX_VIEWS];  // views[r] for rules 1 .. n_views
    int n_views = 0;
    spk::DevBuf<int32_t> pvl, pvr;     // view positions of pairs [pv_base, n_pairs)
    int64_t pv_base = 0;
    // Every change of the pair set goes through these three (spk_ctx.hip), so that each path invalidates the same
    // things: there is no pair set (and so no codes); pl / pr now hold n pairs of a new set; the new set's rules
    // start at the ordinals rule_base and it has n_out pairs (no rules: a loaded pair list).
    void pairs_dropped();
    void pairs_replaced(int64_t n);
    void set_rule_ranges(const std::vector<int64_t> &rule_base, int64_t n_out);
    // the last spk_block_residual: key candidates it enumerated on this shard (after the link-type predicate and
    // the exclusion by earlier key-only rules), -1 = none yet; device milliseconds of its compaction (timing on:
    // the sum of the intervals around each rule's count kernel + scan and around the emit kernels), -1 = none
    int64_t res_enumerated = -1;
    double res_filter_ms = -1.0;

    // packed comparison-vector codes
    spk::DevBuf<uint8_t> codes;
    int code_bytes = 2;
    int K = 0;
    std::vector<int32_t> n_levels;
    std::vector<int64_t> stride;
    int64_t n_patterns = 0;
    bool codes_valid = false;
    int64_t last_deferred = 0;
    std::vector<int64_t> last_exact;  // per column: pairs the last spk_gammas evaluated exactly
    std::vector<int64_t> last_implied;  // per column: pairs whose level the blocking key implied
    int filter_mode = 1;              // 1: template-shaped columns through the filter kernel (spk_filter.hip),
                                      // 0: every column through the interpreter (spk_gammas_set_simple)
    int use_views = 1;                // rule 1's pairs read a view-ordered row image: 0 never, 1 when the
                                      // image outgrows the caches, 2 always (tests)
    int64_t last_view_regions = 0;    // filter regions the last spk_gammas ran as a view launch
    int last_simple = 0;
    // ordinal windows: spk_gammas runs the filter / exact / slow passes over windows of at most this many
    // pairs (0: the default, just under 2^31 -- the work lists hold window-relative int32 ordinals); each
    // window but the last is settled before the next one reuses the lists
    int64_t gamma_window = 0;
    int64_t last_windows = 0;             // windows the last spk_gammas ran
    std::vector<int64_t> exact_carry;     // exact-pass cells of the windows settled before the last one
    int64_t deferred_carry = 0;           // their slow-list cells
    // their exact lists (spk_gammas_exact_list), copied behind each other into xcarry when a window is settled:
    // the next window reuses the slot's list buffer
    struct ListSeg {
        int k;                 // column
        int64_t first, off, n; // the window's first pair ordinal; the list's place in xcarry and its length
    };
    std::vector<ListSeg> list_carry;
    spk::DevBuf<int32_t> xcarry;
    int64_t xcarry_used = 0;

    // comparison-vector buffers shared by every window (reused across calls)
    spk::DevBuf<uint8_t> img[2];      // filter row images of table 0 / table 1
    std::vector<int64_t> img_key[2];  // what img[s] was built from: table version, rows, column layout
    spk::DevBuf<uint8_t> vimg[spk::MAX_VIEWS][2];  // row images in rule-view order (views[r])
    std::vector<int64_t> vimg_key[spk::MAX_VIEWS][2];
    uint64_t table_epoch = 0;
    spk::DevBuf<uint8_t> prog_blob;   // comparison programs, literals, strides (uploaded when they change)
    std::vector<uint8_t> last_blob;   // host copy of what prog_blob holds
    // per column: whether the last settled spk_gammas found cells on its slow list; with the same pairs,
    // tables and program the next call does not launch the slow-list kernels of columns that had none
    // (settle_gammas runs them if the list is not empty after all)
    std::vector<uint8_t> slow_seen;
    bool slow_seen_valid = false;
    bool lev_bag = true;           // k_compact_lev's bag-distance decisions before a refill pass (mode 3: off)
    int lev_kernel = 2;            // Levenshtein exact pass: 0 k_gamma_exact_simple<X_LEV>, 1 k_lev_refill, 2 refill in
                                   // free-text columns (rows past 64 units), one cell per lane elsewhere
    int lev_bound = 1;             // filter field of template Levenshtein columns without free-text rows: 1 the positional
                                   // sketch (two-segment bound), 0 key, lengths and whole-string sketch (spk_gammas_set_lev_bound)
    bool slow_force_skip = false;  // tests: leave every slow-list launch to settle_gammas
    uint64_t slow_key_pairs = 0, slow_key_tables = 0;

    // The state of one ordinal window of spk_gammas: its list buffers, info block and pinned readback, plan, the
    // stream it runs on and the events on that stream.  Consecutive windows reuse slot[0], each settled before the
    // next.  A two-stream split (spk_gammas_set_streams: a pair set that fits one window but holds at least
    // split_min pairs) runs window 0 in slot[0] and window 1 in slot[1] at once, so one window's filter (texture-
    // address bound) shares the CUs with the other's exact passes (VALU bound).  slot[0].stream is the context
    // stream, taken at the start of each call (spk_ctx_set_stream can change it); slot[1] owns its stream.  The
    // phase, slow-list and settle functions take the slot they work on; nothing is exchanged during a call.
    struct Slot {
        spk::DevBuf<int32_t> work;
        spk::DevBuf<int32_t> xlist;       // [2 x xcap]: compacted exact-pass lists, column after column | slow lists
        spk::DevBuf<int64_t> xpref;       // [K][regions + 1] offsets of each region's list in its column's list
        spk::DevBuf<int64_t> xinfo;       // [col_base K | col_count K | overflow | total] (k_prefix)
        spk::DevBuf<unsigned int> region_count;  // [K][regions] filter work-list lengths
        int64_t xcap = 0;
        spk::PinnedBuf<int64_t> h_info;   // pinned readback of xinfo + slow counts
        hipEvent_t ev_info = nullptr;     // after the info-block readback
        // the window's plan (its arguments, what its settlement read), and whether its info block still has to be
        // read (settle_gammas, at the next synchronisation of a consumer)
        spk::GammaPlan *gplan = nullptr;
        bool gamma_pending = false;
        hipStream_t stream = nullptr;
        // per comparison column: HIP events around its exact-pass launch in this window (timing on; the fused
        // Jaro-Winkler launch is shared by its columns)
        std::vector<hipEvent_t> xev0, xev1;
        std::vector<char> xev_used;
    } slot[2];
    int last_slots = 0;        // slots the last spk_gammas used (2: it ran split)
    spk::GammaCols *gcols = nullptr;  // the last spk_gammas' column decisions, shared by its windows
    int gamma_streams = 2;
    int64_t split_min = (int64_t)1 << 22;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    bool split_ready = false;  // slot[1]'s stream and the events exist
    // The pass's launches as a captured HIP graph (spk_gammas_set_graph, off by default): a call whose key -- program,
    // pairs, tables, buffers, window layout, slow-list decisions -- equals the previous call's is captured, later
    // calls with that key replay it (one launch instead of ~25 API calls).  Measured slower than direct launches
    // on MI355X (cfg2 0.939 -> 0.954 ms per step, profiles/r6_ab_gamma_graph.log), so it is opt-in.
    bool use_graph = false;
    hipGraph_t graph = nullptr;
    hipGraphExec_t gexec = nullptr;
    std::vector<int64_t> gkey, gkey_prev;
    std::vector<char> gskip[2];        // the slots' slow_skipped at capture
    int64_t gview_regions = 0;
    int64_t graph_launches = 0;        // replays so far (diagnostics)

    // EM state
    spk::DevBuf<uint64_t> hist;
    spk::DevBuf<double> mpat, llpat, cpat, stats, mu;  // per pattern: mp, ln(...), count; statistics; m / u
    spk::DevBuf<unsigned int> em_ticket;  // k_em_iter's last-workgroup ticket (kept zero between launches)
    spk::DevBuf<uint32_t> em_row;         // its reduction rows (kept zero between launches)
    spk::DevBuf<int32_t> em_hot;          // the pattern it does not count with R < 64 lane copies (-1: none yet)
    std::vector<int64_t> em_hot_key;      // the pair set / pattern space it was found for
    spk::PinnedBuf<double> h_stats;   // pinned host copy of the statistics vector
    int n_cu = 256;                   // compute units of the device (grid sizing)
    int lds_per_block = 64 * 1024;    // LDS a workgroup may allocate (device attribute)
    spk::DevBuf<double> mp;  // per-pair scores (final E-step)
    // tf_adjusted_match_prob kept on the device (spk_tf_apply* with out_tf_mp = NULL): pairs [tf_start, tf_start +
    // tf_count) of the pair set tf_epoch (pairs_epoch then); read back by range with spk_tf_copy
    spk::DevBuf<double> tf_mp;
    int64_t tf_start = 0, tf_count = -1;
    uint64_t tf_epoch = 0;
    // mp per pattern of the last spk_score (the tf sums read it): a table of its own, since every EM
    // launch rewrites mpat with its iteration's parameters
    spk::DevBuf<double> mpat_score;
    std::vector<spk::RawCol *> raw;  // device copies of the input columns (spk_raw_*)
    ~spk_ctx();  // spk_gamma.hip, where the plans are complete types
    bool mpat_valid = false;  // mpat_score holds the mp per pattern of the current codes' last spk_score
    uint64_t score_seq = 0;   // spk_score calls so far (the tf runs depend on their mp per pattern)
    // spk_select: the last selection's survivors, and the code corrections settle_gammas has made so far (a selection
    // taken before one is stale)
    spk::Selection sel;
    uint64_t codes_fix_seq = 0;
    // the last spk_select_best (spk_best.hip): survivors before, pairs kept (-1: none, or it failed), device milliseconds
    int64_t best_before = -1, best_kept = -1;
    double best_ms = -1.0;
    // the last spk_select_sample (spk_select.hip): per stratum the eligible pairs and the pairs kept (empty: none, or it
    // failed), device milliseconds
    std::vector<int64_t> strata_pop, strata_kept;
    double strata_ms = -1.0;
    // the last spk_select_top / spk_select_top_of (spk_select.hip): eligible pairs, pairs kept, pairs at the cut and
    // how many of them are kept (-1 each: none, or it failed), the cut score (NaN: no cut, or a NULL cut), device milliseconds
    int64_t top_eligible = -1, top_kept = -1, top_tied = -1, top_tied_kept = -1;
    double top_cut = __builtin_nan(""), top_ms = -1.0;
    // spk_components*: the last labels
    spk::Components comp;
    // spk_components_sweep*: the last sweep, and which edges a level's rounds hook: 0 the level's new edges plus a star
    // edge per node, 1 every edge up to the level (spk_components_sweep_set_mode)
    spk::ComponentSweep sweep;
    int sweep_mode = 0;
    bool metrics_edge_agg = true;  // spk_cluster_metrics' edge pass counts inside the wave (spk_cluster_metrics_set_mode 0: off)
    // the last spk_label_histogram (spk_labels.hip): pairs counted (-1: none, or it failed), device milliseconds of
    // its launches; its buffers live for the call only
    int64_t label_pairs = -1;
    double label_ms = -1.0;
    // the last spk_label_scores_* (spk_labels.hip): the same two numbers; its buffers live for the call only
    int64_t score_pairs = -1;
    double score_ms = -1.0;
    // the last spk_label_pairs_histogram (spk_labels.hip): pairs counted and device milliseconds as above, the slots of
    // its hash table and the longest insert probe (all -1: none, or it failed); its buffers live for the call only
    int64_t lpairs_pairs = -1, lpairs_capacity = -1;
    double lpairs_ms = -1.0;
    int lpairs_max_probe = -1;
    // the last spk_label_pairs_scores_* (spk_labels.hip): the same four numbers; its buffers live for the call only
    int64_t lpscore_pairs = -1, lpscore_capacity = -1;
    double lpscore_ms = -1.0;
    int lpscore_max_probe = -1;
    // the last spk_cluster_agreement (spk_agreement.hip): levels it scored (-1: none yet), device milliseconds of its
    // launches; a failing call leaves both as they were, and its buffers live for the call only
    int agree_levels = -1;
    double agree_ms = -1.0;
    // the last spk_pairs_sample (spk_sample.hip): draws generated and pairs kept (-1: none, or it failed), device
    // milliseconds of its launches
    int64_t sample_draws = -1, sample_kept = -1;
    double sample_ms = -1.0;
    // the last spk_block_profile (spk_block.hip): ordinals its count pass enumerated (-1: none, or it failed), HIP-event
    // milliseconds of its key-level part and of its enumeration (timing on, else -1); its buffers live for the call
    // only.  profile_cut: the largest-blocks step sorts only the blocks of the top bins (0: every block)
    int64_t profile_ordinals = -1;
    double profile_key_ms = -1.0, profile_enum_ms = -1.0;
    bool profile_cut = true;
    // the (value, pattern) runs of the last tf scale pass over a device-id column, reused by its sum pass
    spk::DevBuf<unsigned long long> tf_uniq;
    spk::DevBuf<unsigned int> tf_runs, tf_nruns;
    // or, when n_values x n_patterns is small enough, the (value, pattern) pair counts themselves (tf_pass)
    spk::DevBuf<unsigned long long> tf_hist;
    spk::DevBuf<uint8_t> tf_sort;  // the sort form's keys, sorted keys and sort scratch (scale pass to sum pass)
    std::vector<int64_t> tf_key;
    int tf_mode = 0;  // spk_tf_set_mode: 0 auto (histogram when it fits), 1 always the sort, 2 the sort with 64-bit keys
    int ingest_hash_bits = 63;  // spk_ingest_set_hash_bits: width of hashed_ids' hash (tests force collisions below 63)
    bool hist_lanes = true;  // k_hist_lanes (lane-private LDS counters) when the pattern space fits
    bool em_fence = true;    // k_em_iter: release fence before each ticket (spk_em_set_lane_histogram 2: none)

    // asynchronous EM iteration (spk_em_iteration_start / _wait): the statistics land in h_stats behind
    // ev_stats; the arguments are kept so that the launch can be repeated when the codes it read are
    // corrected after spk_gammas returned (settle_gammas -> em_requeue)
    bool em_pending = false;
    uint64_t gamma_seq = 0;           // spk_gammas calls so far (the codes' generation)
    uint64_t em_seq = 0;              // the generation the pending EM iteration read
    double em_lambda = 0.0, em_one_minus = 0.0;
    std::vector<double> em_m, em_u;
    int em_n_stats = 0;
    int em_kind = 0;                  // 0: one-launch iteration (re-enqueued on a code fix), 1: finalize of a
                                      // caller's (all-reduced) histogram, whose codes were settled before
    hipEvent_t ev_stats = nullptr;    // after the EM statistics readback

    // timing: two event pairs per kind, alternating, so the last completed launch of a kind can be read
    // while a newer one is still in flight (spk_ctx_kernel_ms_done)
    bool timing = false;
    bool timing_exact = false;  // also each column's exact-pass launch (spk_ctx_enable_timing 2): events cost host time per launch
    hipEvent_t ev0[2][spk::K_COUNT] = {}, ev1[2][spk::K_COUNT] = {};
    bool ev_used[2][spk::K_COUNT] = {};
    int ev_slot[spk::K_COUNT] = {};
    // the one event pair of the stages that run after scoring (spk::StageTimer), created on first use with timing on
    hipEvent_t stage_ev0 = nullptr, stage_ev1 = nullptr;

    // HIP events around column k's exact-pass launch in a window (timing_exact)
    int xbegin(Slot &s, int k);
    int xend(Slot &s, int k);

    int begin(spk::Kern k);
    int end(spk::Kern k);
    spk::Table &side_table(int operand_side) { return table[(operand_side == 1 && link_type == SPK_LINK_ONLY) ? 1 : 0]; }
};

namespace spk {
inline bool Selection::current(const spk_ctx *ctx) const {
    return ctx->codes_valid && pairs_epoch == ctx->pairs_epoch && gamma_seq == ctx->gamma_seq &&
           fix_seq == ctx->codes_fix_seq;
}

// The node ids of the context's link type, as spk_select_best and spk_components* number them: the l side's input rows
// are [0, n0), the r side's [r_base, r_base + n1).  Not link_only: both sides are table 0 and r_base = 0.  A table
// that is not loaded has n = -1; the caller checks n0 and n1 under its own name before it uses the rest.
struct NodeSpace {
    const Table *t0, *t1;
    int64_t n0, n1, r_base, n_nodes;
};
inline NodeSpace node_space(spk_ctx *ctx) {
    const Table &t0 = ctx->table[0], &t1 = ctx->side_table(1);
    const bool two = ctx->link_type == SPK_LINK_ONLY;
    return NodeSpace{&t0, &t1, t0.n, t1.n, two ? t0.n : 0, t0.n + (two ? t1.n : 0)};
}

// HIP-event stopwatch of a stage that runs after scoring, over the context's one event pair: the sum of the intervals
// between open() and close().  One pair is enough because every user is a top-level entry that has read its last
// interval, behind a stream synchronisation, before it returns, and none calls another while an interval is open
// (pattern_mp_table and the residual path's gamma pass time themselves with ev0 / ev1[K_*]).  With timing off
// nothing is created or recorded.
struct StageTimer {
    spk_ctx *ctx;
    double ms = 0.0;
    enum { IDLE, OPEN, STOPPED } state = IDLE;
    int open() {  // starts an interval unless one is open already
        if (!ctx->timing || state != IDLE) return SPK_OK;
        if (!ctx->stage_ev0) SPK_HIP(hipEventCreate(&ctx->stage_ev0));
        if (!ctx->stage_ev1) SPK_HIP(hipEventCreate(&ctx->stage_ev1));
        SPK_HIP(hipEventRecord(ctx->stage_ev0, ctx->stream));
        state = OPEN;
        return SPK_OK;
    }
    // The two halves of close(), for a caller that enqueues read-backs behind the interval's end and synchronises
    // itself (scan_total): stop() ends the open interval, add() follows the synchronisation.
    int stop() {
        if (state != OPEN) return SPK_OK;
        SPK_HIP(hipEventRecord(ctx->stage_ev1, ctx->stream));
        state = STOPPED;
        return SPK_OK;
    }
    int add() {
        if (state != STOPPED) return SPK_OK;
        float t = 0.f;
        SPK_HIP(hipEventElapsedTime(&t, ctx->stage_ev0, ctx->stage_ev1));
        ms += (double)t;
        state = IDLE;
        return SPK_OK;
    }
    int close() {  // ends the open interval, synchronises the stream (with timing off too), adds the interval
        SPK_TRY(stop());
        SPK_HIP(hipStreamSynchronize(ctx->stream));
        return add();
    }
    double result() const { return ctx->timing ? ms : -1.0; }  // what the *_info calls report
};

// spk_components.hip, also for spk_bridges.hip: label [n_nodes] (the caller's device words) = the smallest node id of
// each node's component in the graph (eu, ev) [n_edges], by k_cc_init and the components' round loop.  eu and ev start
// 16-byte aligned (k_cc_hook's loads).  bad_code / bad_msg: an id >= n_nodes; limit_msg: the round cap.  T may be open.
int components_of_edges(spk_ctx *ctx, int64_t n_nodes, int64_t n_edges, const uint32_t *eu, const uint32_t *ev,
                        uint32_t *label, int bad_code, const char *bad_msg, const char *limit_msg, StageTimer &T,
                        int *out_rounds, int64_t *out_n_clusters);

int ensure_desc(spk_ctx *ctx, Table &t);
// Finishes the last spk_gammas (work-list overflow, huge pass) once the stream is synchronised;
// *fixed = true when codes changed after spk_gammas returned.  No-op when nothing is pending.
int settle_gammas(spk_ctx *ctx, bool *fixed);
// Enqueue the pending asynchronous EM iteration again (its codes were corrected after it was enqueued).
int em_requeue(spk_ctx *ctx);
// mp per pattern of the current pattern space into d_mpat [n_patterns] (device), with spk_score's own arguments
// and kernel (pat_args, k_pattern_mp), enqueued on the context stream.  Writes no context state but the m / u
// staging buffer of large tables.
int pattern_mp_table(spk_ctx *ctx, double lambda, double one_minus, const double *m, const double *u, double *d_mpat);
int new_column(spk_ctx *ctx, int side, int col, Column **out);
int launch_unit_bits(spk_ctx *ctx, int64_t n, Column *c);
int build_bag_rows(spk_ctx *ctx, int64_t n, Column *c);
int build_pos_rows(spk_ctx *ctx, int64_t n, Column *c);
int launch_utf8_decode(spk_ctx *ctx, int64_t n, const int64_t *off8, const int64_t *src_off, const int32_t *perm,
                       const uint8_t *bytes, const uint8_t *valid, Column *c, bool long_rows, const int64_t *ids);
}
