/*
 * splink_hip.h -- C ABI of libsplink_hip.so, the MI355X (gfx950) execution engine for
 * splink's pairwise-comparison + EM hot path.
 *
 * The reference (splink 0.1.7) has no native boundary: every stage is a Python
 * function that emits Spark SQL.  These entry points replace the
 * Spark execution (L0) of those stages; the Python layer in splink_amd/ keeps the
 * reference's stage-function API and calls them through ctypes.  Each entry point
 * names the reference interface it replaces.
 *
 * Conventions
 *   - Every function returns SPK_OK (0) or a negative SPK_E_* code; spk_last_error()
 *     gives a thread-local message.
 *   - Host buffers passed in are BORROWED for the duration of the call; outputs are
 *     caller-allocated.  Device state is owned by the context.
 *   - A context is bound to one HIP device and one stream and is not re-entrant;
 *     callers serialise.  Multi-GPU = one process (one context) per GPU; the only
 *     cross-GPU exchange is the EM pattern histogram (spk_em_histogram writes it to a
 *     caller-provided device buffer, the caller all-reduces it, spk_em_finalize reads it).
 */
#ifndef SPLINK_HIP_H
#define SPLINK_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPK_OK 0
#define SPK_E_INVALID (-1) /* bad argument / shape (Python: ValueError) */
#define SPK_E_HIP (-2)     /* HIP runtime failure */
#define SPK_E_OOM (-3)     /* device allocation failed */
#define SPK_E_STATE (-4)   /* call out of order (e.g. gammas before pairs) */
#define SPK_E_LIMIT (-5)   /* input beyond a supported limit (e.g. 2^31 rows in one table) */

#define SPK_LINK_DEDUPE 0        /* "dedupe_only"     */
#define SPK_LINK_ONLY 1          /* "link_only"       */
#define SPK_LINK_AND_DEDUPE 2    /* "link_and_dedupe" */

typedef struct spk_ctx spk_ctx;

const char *spk_last_error(void);
int spk_version(void);
int spk_device_count(int *out);

/* ---- context ------------------------------------------------------------------ */
int spk_ctx_create(int device, spk_ctx **out);
void spk_ctx_destroy(spk_ctx *ctx);
/* Run all work on `hip_stream` (a hipStream_t; NULL = the context's own stream). */
int spk_ctx_set_stream(spk_ctx *ctx, void *hip_stream);
int spk_ctx_sync(spk_ctx *ctx);
/* Link type of the loaded tables (needed before spk_pairs_load / spk_gammas when spk_block is not used). */
int spk_ctx_set_link_type(spk_ctx *ctx, int link_type);
/* Elapsed milliseconds of the last launch of each kernel family, measured with HIP events
 * on the context stream: [0] block, [1] gamma, [2] em_hist, [3] em_final, [4] score. */
int spk_ctx_kernel_ms(spk_ctx *ctx, double *out5);
/* The same without synchronising: per family the newest launch that has completed (-1 = none), so a
 * caller can read the timings of iteration i while iteration i + 1 is still queued. */
int spk_ctx_kernel_ms_done(spk_ctx *ctx, double *out5);
/* on = 1: HIP events around each kernel family (spk_ctx_kernel_ms); on = 2: also around each column's exact-pass
 * launch (spk_gammas_exact_ms); 0: off. */
int spk_ctx_enable_timing(spk_ctx *ctx, int on);
/* LDS bytes one workgroup may allocate on the context's device (sizes the E/M histogram copies). */
int spk_ctx_lds_per_block(spk_ctx *ctx, int *out);
/* Device memory the context holds, by what it stores (bytes allocated): [0] raw input columns (Arrow
 * buffers as handed over), [1] record encodings (decoded columns: units, metadata, bit-planes, bag rows,
 * numeric values; row permutations, ranks, blocking keys), [2] filter row images, [3] candidate pairs (row
 * indices, rule-view positions and rows), [4] comparison codes, [5] comparison work lists (filter lists,
 * exact / slow lists, region counts), [6] EM, scoring and tf state, the last selection (spk_select, spk_select_best) and the last
 * components' labels (spk_components*), the last sweep with its metrics (spk_components_sweep*), [7] the sum.  For sizing a share of a
 * job against a device's memory (there is no reference counterpart: Spark spills). */
int spk_ctx_memory(spk_ctx *ctx, int64_t *out8);

/* ---- record tables (replaces createOrReplaceTempView of df / df_l / df_r,
 *      blocking.py:209-222, and the vertical concatenation of :70-93) ------------ */
/* side 0 = df (dedupe_only, link_and_dedupe after concatenation) or df_l; side 1 = df_r. */
int spk_table_create(spk_ctx *ctx, int side, int64_t n_rows, int n_cols);
/* String column from Arrow-style UTF-8: offsets[n_rows+1] into data; valid[n_rows] (1 = non-null).
 * Decoded on the device to UTF-16 code units (Jaro-Winkler alphabet) + code-point lengths.
 * value_ids (optional, may be NULL): a dictionary id per row, equal iff the strings are equal, in
 * one id space for side 0 and side 1 (Arrow dictionary encoding), in [0, 2^32) for non-NULL rows.
 * With ids, string equality in comparison programs is one integer compare; without, a hash then
 * a unit compare.  A column holds at most 2^34 UTF-16 units. */
int spk_table_add_utf8(spk_ctx *ctx, int side, int col, const int64_t *offsets, const uint8_t *data,
                       const uint8_t *valid, const int64_t *value_ids);
int spk_table_add_float64(spk_ctx *ctx, int side, int col, const double *values, const uint8_t *valid);
/* Order rank per row for the link-type predicate: dedupe `l.uid < r.uid` (blocking.py:136),
 * link_and_dedupe `(l.src < r.src) or (l.uid < r.uid and same src)` (:139).  Equal rank = equal key.
 * Per-row host arrays (rank, keys) are in INPUT row order; after spk_cluster they are taken through the
 * table's permutation.  A new rank clears the NULL-id layout (declare it again with spk_table_set_rank_null). */
int spk_table_set_rank(spk_ctx *ctx, int side, const int64_t *rank);
/* NULL unique ids (blocking.py:136, :139: `l.uid < r.uid` is NULL, so the pair is dropped, unless
 * `l._source_table < r._source_table` holds).  divisor > 0 declares the rank layout
 * rank = source * divisor + r with r = divisor - 1 for a row whose unique id is NULL; 0 = no NULL ids. */
int spk_table_set_rank_null(spk_ctx *ctx, int side, int64_t divisor);
/* Blocking key ids of rule `rule` for each row (-1 = NULL: the row never matches the rule).
 * which = 0: key of the row as the join's l-side; which = 1: as the r-side. */
int spk_table_set_key(spk_ctx *ctx, int side, int rule, int which, const int64_t *keys);

/* ---- device ingest (replaces the per-row key / value preparation that Spark does inside the
 *      equi-joins of blocking.py:95-160 and the projections of gammas.py:65-89) ----------------
 * Input columns are handed over once as Arrow buffers ("raw" columns, input row order, indexed by
 * `raw`, borrowed for the call).  Everything derived from them is computed on the device. */
int spk_raw_utf8(spk_ctx *ctx, int raw, int64_t n, const int64_t *offsets, const uint8_t *data, const uint8_t *valid);
/* The same from Arrow buffers as they are (zero-copy on the host side): `offsets` (n + 1, any base: a
 * sliced array's first offset may be past 0), `data` the value buffer those offsets index, `validity`
 * the Arrow validity bitmap (LSB first, from bit validity_bit_offset; NULL = no NULLs; offset -1: one byte
 * per row instead, 0 = NULL).  on_device = 1:
 * all three are device pointers (e.g. rows all-gathered from the ranks that uploaded them) and are
 * copied device to device.  Rebasing, validity expansion and the length scan run on the device. */
int spk_raw_utf8_arrow(spk_ctx *ctx, int raw, int64_t n, const int64_t *offsets, const uint8_t *data,
                       const uint8_t *validity, int64_t validity_bit_offset, int on_device);
/* A chunked Arrow column (pyarrow ChunkedArray: one call instead of a host-side combine_chunks copy):
 * chunk c has rows[c] rows, its own offsets (any base), data and validity (bit_offsets[c] as above, -1 for
 * one byte per row; validity[c] NULL = no NULLs).  The chunks' rows are concatenated in order. */
int spk_raw_utf8_arrow_chunks(spk_ctx *ctx, int raw, int n_chunks, const int64_t *rows, const int64_t *const *offsets,
                              const uint8_t *const *data, const uint8_t *const *validity, const int64_t *bit_offsets);
/* 64-bit digest of a table's encoded device form (row permutation, ranks, every comparison column's
 * metadata / bit-planes / values, blocking keys): two contexts that ingested the same rows by
 * different routes (local upload, or rows gathered from other ranks) give the same digest. */
int spk_table_digest(spk_ctx *ctx, int side, uint64_t *out);
/* Free a raw column's device buffers (its keys and decoded columns stay; using it again is SPK_E_STATE
 * until it is uploaded again under the same index). */
int spk_raw_release(spk_ctx *ctx, int raw);
/* 8-byte values compared as bit patterns (int64 ids, canonical float64 bits, host-computed key ids). */
int spk_raw_i64(spk_ctx *ctx, int raw, int64_t n, const int64_t *values, const uint8_t *valid);
/* One equality term of a blocking rule: l-side column `raw_l` (table 0) = r-side column `raw_r` (the
 * r table; -1 = the same column, a symmetric term), each with an optional Spark substr(start, len)
 * on code points (len < 0 = none). */
typedef struct {
    int32_t raw_l, raw_r;
    int32_t l_substr_start, l_substr_len;
    int32_t r_substr_start, r_substr_len;
} spk_key_term;
/* Blocking key of rule `rule` (the conjunction of its terms; NULL if a term is NULL): hash, radix sort
 * and verified dense ids on the device, one id space for both sides.  Same result as
 * spk_table_set_key with host-computed ids (which stays available for other key expressions). */
int spk_key_build(spk_ctx *ctx, int rule, int n_terms, const spk_key_term *terms);
/* Width of the hash behind the dense ids of spk_key_build and spk_table_add_raw_utf8: 1 .. 63 bits, 63 by
 * default (then the ids are what they were without this call).  A test knob: at a few bits values collide,
 * which reaches the byte-for-byte verification, the retry under the next of four seeds and the SPK_E_STATE
 * return after the fourth.  Which values share an id does not depend on the width (the ids' order does). */
int spk_ingest_set_hash_bits(spk_ctx *ctx, int bits);
/* Rank for the link predicate from int64 unique ids (raw column, NULL allowed): dense rank, rows
 * [right_from, n) being the 'right' source of link_and_dedupe (-1 = none).  Also sets the NULL-id
 * layout of spk_table_set_rank_null. */
int spk_rank_from_raw(spk_ctx *ctx, int raw_uid, int64_t right_from);
/* Reorder the tables' rows by rule 0's key, then rank (NULL keys last), so a block's rows are
 * contiguous on the device.  Keys and ranks move with the rows; comparison columns must be added
 * after this (they are decoded through the permutation); keys built and ranks set after it follow the
 * table's row order too (calling it again composes the permutations).  out_perm0 / out_perm1 (host,
 * optional): input row of each table row. */
int spk_cluster(spk_ctx *ctx, int32_t *out_perm0, int32_t *out_perm1);
/* String comparison column `col` from raw column raw0 (table 0) and, for link_only, raw1 (table 1):
 * decoded to UTF-16 through the tables' row permutations, with dictionary ids computed on the
 * device in one id space for both sides. */
int spk_table_add_raw_utf8(spk_ctx *ctx, int col, int raw0, int raw1);

/* ---- blocking (replaces block_using_rules / cartesian_block, blocking.py:162-318) -- */
/* Generates candidate pairs for rules 0..n_rules-1 in order, each excluding pairs an earlier
 * rule matched (`AND NOT ifnull(rule_j, false)`, :59-68), with the link-type predicate.
 * rule_symmetric[r] = 1 when the rule's l- and r-side keys are the same function of a row.
 * Pairs are generated for the shard [shard/n_shards] of the global candidate-ordinal space
 * and stay on the device (int32 row indices). */
int spk_block(spk_ctx *ctx, int link_type, int n_rules, const int32_t *rule_symmetric, int shard,
              int n_shards, int64_t *out_n_pairs, int64_t *out_n_candidates_total);
int spk_pairs_count(spk_ctx *ctx, int64_t *out);
int spk_pairs_copy(spk_ctx *ctx, int64_t start, int64_t count, int32_t *out_l, int32_t *out_r);
/* Use caller-provided pairs (e.g. add_gammas on an externally built comparison frame). */
int spk_pairs_load(spk_ctx *ctx, int64_t n, const int32_t *rows_l, const int32_t *rows_r);
/* Random record pairs, drawn on the device (no counterpart in the reference release; later releases:
 * estimate_u_using_random_sampling).  Replaces the pair set by the surviving draws among the ordinals
 * [first_draw, first_draw + n_draws) of a sample of total_draws, in ordinal order; like a loaded list the set has
 * no rules, no views and no key terms, and spk_gammas follows as usual.  Draw i is a function of (seed, i,
 * total_draws, the table sizes, the ranks) only -- not of the range, the grid or the launch shape -- so the
 * concatenation of the results over any partition of [0, total_draws) into ranges is the whole sample.  The draws
 * are independent: this is sampling WITH replacement, the same pair may occur more than once (about
 * N^2 / (2 * pairs) duplicates among N draws from `pairs` possible pairs).
 *
 * Definition (all arithmetic mod 2^64; n0, n1 the row counts of table 0 and table 1; rank as spk_table_set_rank):
 *   mix(x):      x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB; x ^= x >> 31
 *                (the splitmix64 finaliser)
 *   word(i, j) = mix(mix(seed) + 0x9E3779B97F4A7C15 * (3 * i + j + 1)),  j = 0, 1, 2
 *   below(w, n) = (w * n) >> 64  (the high 64 bits of the 128-bit product)
 *   anchor (stratified: draw i's anchor lies in the i-th of total_draws equal slices of table 0, so the anchors are
 *   non-decreasing in i and the anchor side of the comparison pass streams through the table):
 *     lo = (i * n0) / total_draws,  hi = ((i + 1) * n0) / total_draws  (exact integer quotients)
 *     a = lo + below(word(i, 0), hi - lo) when hi > lo, else a = lo
 *   link_only:  b = below(word(i, 1), n1); the pair is (l, r) = (a, b), a row of table 0 and a row of table 1.  Every
 *     draw survives.  No pairs when n0 = 0 or n1 = 0.
 *   dedupe_only, link_and_dedupe (one table):  b = below(word(i, 1), n0 - 1), then b += (b >= a).  The pair is the two
 *     rows ordered by rank, the lower rank as l.  The draw is dropped when the ranks are equal, and under the
 *     NULL-unique-id rule of spk_block (spk_table_set_rank_null with divisor d > 0: dropped when rank(l) / d ==
 *     rank(r) / d and either rank % d == d - 1).  Every sampled pair is thus one the blocking of no rules (the
 *     cartesian product under the link-type predicate) produces.  No pairs when n0 < 2.
 *   word(i, 2) is reserved: nothing reads it now, so a later per-draw decision does not move the pairs.
 *
 * SPK_E_STATE: tables not loaded, or no rank under dedupe_only / link_and_dedupe.  SPK_E_INVALID: a negative
 * total_draws, first_draw or n_draws, or a range that ends past total_draws.  SPK_E_LIMIT: total_draws * n0 does not
 * fit in 63 bits.  A failing call leaves no pair set. */
int spk_pairs_sample(spk_ctx *ctx, int link_type, uint64_t seed, int64_t total_draws, int64_t first_draw,
                     int64_t n_draws, int64_t *out_n_pairs);
/* The last spk_pairs_sample: draws generated and pairs kept (-1 each: none yet, or the last call failed), and with
 * timing on (spk_ctx_enable_timing) the device milliseconds of its launches (count kernel, scan, emit kernel),
 * -1 otherwise. */
int spk_pairs_sample_info(spk_ctx *ctx, int64_t *out_draws, int64_t *out_kept, double *out_ms);

/* ---- comparison programs (replaces add_gammas / the CASE templates,
 *      gammas.py:65-124, case_statements.py:62-277) ----------------------------- */
/* Operand of a predicate: a column of the pair's l- or r-record, or a literal, with an
 * optional ifnull() default and an optional substr(start, len) (code points, Spark rules). */
typedef struct {
    int32_t kind;        /* 0 column, 1 string literal, 2 number literal */
    int32_t side;        /* 0 = `_l` record, 1 = `_r` record */
    int32_t col;         /* column index in the side's table */
    int32_t lit;         /* string literal index (kind 1) or ifnull default string (-1 none) */
    double num;          /* number literal (kind 2) or ifnull default number */
    int32_t has_num_default;
    int32_t substr_start; /* 1-based Spark substr position; 0 = no substr */
    int32_t substr_len;
    int32_t pad;
} spk_operand;

/* Predicate instruction (RPN over Kleene booleans). */
#define SPK_OP_ISNULL 1     /* a IS NULL */
#define SPK_OP_NOTNULL 2    /* a IS NOT NULL */
#define SPK_OP_STR_CMP 3    /* a cmp b (strings; = / != / < / <= / > / >=, UTF-8 byte order) */
#define SPK_OP_NUM_CMP 4    /* a cmp b (numbers) */
#define SPK_OP_JW 5         /* jaro_winkler_sim(a, b) cmp t */
#define SPK_OP_LEV 6        /* levenshtein(a, b) cmp t */
#define SPK_OP_LEVRATIO 7   /* levenshtein(a,b)/((length(a)+length(b))/2) cmp t */
#define SPK_OP_ABSDIFF 8    /* abs(a - b) cmp t */
#define SPK_OP_PERCDIFF 9   /* abs(a - b)/abs(case when a > b then a else b end) cmp t */
#define SPK_OP_CONST 10     /* constant: i0 = 0 false, 1 true, 2 null */
#define SPK_OP_AND 20
#define SPK_OP_OR 21
#define SPK_OP_NOT 22
#define SPK_OP_LEN 11       /* length(a) cmp t */
/* The set / token measures of the reference's UDF jar (jars/scala-udf-similarity-0.0.6.jar, registered by name in
 * tests/test_spark.py:44-56), over UTF-16 units as Java Strings; restated from the class files, parity unpinned (the
 * jar is not executable where this was built).  A NULL operand makes either test NULL.
 * jaccard_sim (uk/gov/moj/dash/linkage/JaccardSimilarity.call -> commons-text 1.4 JaccardSimilarity.apply): 0.0 if
 * either string is empty, else Math.round(|A n B| / |A u B| * 100.0) / 100.0 over the sets of distinct units, fp64,
 * round half up.
 * cosine_distance (uk/gov/moj/dash/linkage/CosineDistance.call -> commons-text 1.4 CosineDistance.apply,
 * RegexTokenizer, Counter, CosineSimilarity): tokens are the maximal runs of [A-Za-z0-9_]; 1.0 - dot / (sqrt(d1) *
 * sqrt(d2)) over the per-token counts (cos = 0.0 when a text has no token), not short-cut for equal texts.  A blank
 * text (empty or Character.isWhitespace units only) makes the reference's query throw; here the test is NULL (the one
 * deliberate deviation). */
#define SPK_OP_JACCARD 12   /* jaccard_sim(a, b) cmp t */
#define SPK_OP_COSINE 13    /* cosine_distance(a, b) cmp t */

#define SPK_CMP_EQ 0
#define SPK_CMP_NE 1
#define SPK_CMP_LT 2
#define SPK_CMP_LE 3
#define SPK_CMP_GT 4
#define SPK_CMP_GE 5

typedef struct {
    int32_t op;
    int32_t a, b;   /* operand indices */
    int32_t cmp;    /* SPK_CMP_* */
    int32_t i0;
    int32_t pad;
    double t;       /* threshold */
} spk_instr;

typedef struct {
    int32_t n_levels;    /* L_k; gamma values are -1..L_k-1 */
    int32_t else_level;
    int32_t n_when;
    int32_t first_when;  /* index into the when arrays */
} spk_column_program;

/* Install the comparison programs and evaluate them over the current pairs, producing one
 * packed comparison-vector code per pair: code = Σ_k (γ_k + 1) · Π_{j<k} (L_j + 1).
 * Asynchronous: returns once the passes are queued on the context stream.  A work-list overflow
 * or cells past the exact passes' string limit are completed at the next synchronising call that
 * reads the codes (spk_em_iteration, spk_em_finalize, spk_em_histogram with a caller buffer,
 * spk_score, spk_gammas_copy, the tf calls, spk_ctx_sync), so results are always complete. */
int spk_gammas(spk_ctx *ctx, int n_cols, const spk_column_program *cols, int n_when,
               const int32_t *when_first_instr, const int32_t *when_n_instr, const int32_t *when_level,
               int n_instr, const spk_instr *instr, int n_operands, const spk_operand *operands,
               int n_lits, const int64_t *lit_offsets, const uint8_t *lit_utf8);
/* spk_block for rules with residual predicates: the reference splices any join condition into
 * `on {rule} {not_previous_rules}` (blocking.py:59-68, 145-154), so a rule may AND further conjuncts
 * (`abs(l.age - r.age) < 5`, `levenshtein(l.a, r.a) <= 2`, `l.a != r.a`, `l.age < r.age` ...) onto its key equalities.
 * rule_program[r] = index of rule r's predicate among the column programs given here (spk_gammas' argument
 * format; a 2-level program with ELSE 0 whose level 1 means "the whole rule text is TRUE", i.e.
 * ifnull(rule, false)), or -1 for a rule that is only its key equalities.  At most SPK_MAX_RESIDUAL_RULES
 * programs (3^8 code patterns, inside the 2-byte code); the columns they read must be in the tables.
 * A pair is emitted by rule r iff the link-type predicate holds, rule r is TRUE and every earlier rule is not
 * TRUE (NULL does not emit and does not exclude).  Three steps: (a) spk_block's enumeration of the key candidates,
 * where an earlier rule with a program does not exclude on its key; (b) the programs evaluated over those
 * candidates by the comparison pass; (c) a stable device compaction of the pairs (and the second rule's view
 * positions) by the codes, rule range by rule range, into fresh buffers.  The pair set becomes visible after
 * (c); a failure before leaves none.  The codes of (b) are dropped: spk_gammas must follow as after spk_block.
 * out_n_candidates_total: the key-candidate ordinals, the space the shards are cut on, as spk_block.
 * With every rule_program[r] = -1 the result is spk_block's. */
#define SPK_MAX_RESIDUAL_RULES 8
int spk_block_residual(spk_ctx *ctx, int link_type, int n_rules, const int32_t *rule_symmetric,
                       const int32_t *rule_program, int shard, int n_shards, int n_cols,
                       const spk_column_program *cols, int n_when, const int32_t *when_first_instr,
                       const int32_t *when_n_instr, const int32_t *when_level, int n_instr,
                       const spk_instr *instr, int n_operands, const spk_operand *operands, int n_lits,
                       const int64_t *lit_offsets, const uint8_t *lit_utf8, int64_t *out_n_pairs,
                       int64_t *out_n_candidates_total);
/* The last spk_block_residual: pairs its enumeration produced on this shard before the filter (-1: none yet),
 * and, with timing on, the device milliseconds of its compaction (-1 = none): the sum over HIP event pairs around
 * each rule's count kernel and scan and around the emit kernels; the host round trips between them (survivor
 * counts, buffer allocation) are not in it. */
int spk_block_residual_info(spk_ctx *ctx, int64_t *out_enumerated, double *out_filter_ms);

/* ---- blocking-rule profile (comparison_evaluation.py:12-35 and beyond): what the rules would cost, without
 *      building the pair set ------------------------------------------------------------------------------------ */
typedef struct {
    int64_t rows_l, rows_r;       /* rows with a non-NULL key of the rule as the join's l- / r-side
                                     (symmetric self-join: equal) */
    int64_t blocks;               /* distinct l-side key values among them */
    int64_t candidates;           /* the rule's candidate ordinals: sum over blocks of n(n-1)/2 or nL*nR */
    int64_t largest_candidates;   /* of one block */
    int64_t enumerated;           /* pairs the count pass keeps in this shard's ordinals of the rule,
                                     or -1: not enumerated */
} spk_rule_profile;

typedef struct {
    int64_t rows_l, rows_r, candidates;
    int32_t row_l;                /* table-0 device row of the block's first l-view position */
    int32_t pad;
} spk_block_entry;

#define SPK_PROFILE_BINS 64
#define SPK_LARGEST_BY_CANDIDATES 0
#define SPK_LARGEST_BY_ROWS_L 1

/* Profiles rules 0..n_rules-1 (keys set as for spk_block) from the tables' keys and ranks alone.  Nothing else of the
 * context is read or written: the pair set, views, codes, selection, labels, scores and the context's link type stay,
 * and every buffer of the call is freed before it returns; nothing it allocates is sized by a pair or candidate count.
 *
 * Key-level figures (the same for every shard, O(rows) after the key sort): out_rules' rows_*, blocks, candidates
 * (their sum over the rules is spk_block's out_n_candidates_total) and largest_candidates; the histogram, whose bin i
 * holds the blocks whose candidate count has bit length i (bin 0: a block without a candidate) as
 * out_hist[(r * SPK_PROFILE_BINS + i) * 2 + 0] blocks and [.. + 1] the sum of their candidates; and the first
 * min(limit, blocks) blocks of each rule in descending order of largest_by (candidates or l-side rows), ties by
 * ascending block index in the rule's key order, as out_largest[r * limit + ..] with their number in out_n_largest[r].
 *
 * Enumeration: rule r's ordinals in this shard -- cut as spk_block cuts them -- go through spk_block's count pass when
 * max_enumerate < 0 or the range is at most max_enumerate long (0: never); `enumerated` is then the pairs that pass
 * keeps (the link-type predicate with the NULL-unique-id rule, exclusion on the keys of the earlier rules without a
 * program), else -1.  With rule_program = NULL the sum over the rules is spk_block's out_n_pairs of that shard; with
 * programs (only their sign is read) it is spk_block_residual_info's out_enumerated: residual predicates themselves
 * are not evaluated.  The pass runs in slabs of at most 2^31 ordinals, each reduced to one count on the device.
 *
 * SPK_E_STATE: keys not set for every rule, tables not loaded, no rank under dedupe_only / link_and_dedupe.
 * SPK_E_INVALID: limit < 0, limit > 0 with out_largest or out_n_largest NULL, an unknown largest_by, a bad shard, link
 * type or rule count.  A failing call leaves the outputs unspecified and the context as it was. */
int spk_block_profile(spk_ctx *ctx, int link_type, int n_rules, const int32_t *rule_symmetric,
                      const int32_t *rule_program, int shard, int n_shards, int64_t max_enumerate, int largest_by,
                      int limit, spk_rule_profile *out_rules, int64_t *out_hist, spk_block_entry *out_largest,
                      int32_t *out_n_largest);
/* The last spk_block_profile: with timing on (spk_ctx_enable_timing) the HIP-event milliseconds of its key-level part
 * (sorts, block statistics, largest blocks) and of its enumeration, -1 each otherwise; and the ordinals its count pass
 * went through (-1: no call yet, or the last one failed). */
int spk_block_profile_info(spk_ctx *ctx, double *out_key_ms, double *out_enum_ms, int64_t *out_ordinals_enumerated);
/* Measurement switch: on = 0 makes the largest-blocks step sort every block of a rule instead of only those in the
 * top histogram bins (the default, 1).  The results are the same. */
int spk_block_profile_set_cut(spk_ctx *ctx, int on);
/* Decode codes to int8 gamma columns, [count x K] row-major. */
int spk_gammas_copy(spk_ctx *ctx, int64_t start, int64_t count, int8_t *out);
/* Use a caller-provided gamma matrix (int8 [n x K], values -1..L_k-1).  The pattern space Π (L_k + 1) must be
 * below 2^31 (SPK_E_LIMIT otherwise, as for spk_gammas). */
int spk_gammas_load(spk_ctx *ctx, int n_cols, const int32_t *n_levels, int64_t n, const int8_t *gammas);
int spk_n_patterns(spk_ctx *ctx, int64_t *out);
/* Pairs the last spk_gammas evaluated in the global-memory pass (strings beyond LDS staging). */
int spk_gammas_deferred(spk_ctx *ctx, int64_t *out);
/* Per comparison column: pairs the last spk_gammas could not decide from bounds in the filter pass
 * and evaluated with the exact similarity (out[n], n >= number of columns). */
int spk_gammas_exact_counts(spk_ctx *ctx, int64_t *out, int n);
/* With timing on at level 2 (spk_ctx_enable_timing): milliseconds of each column's exact-pass launch in the last
 * spk_gammas (HIP events; -1 = none; the Jaro-Winkler columns share one launch, reported at the first
 * of them).  Synchronises. */
int spk_gammas_exact_ms(spk_ctx *ctx, double *out, int n);
/* Diagnostics: the first n pair ordinals of column k's exact list of the last spk_gammas (host). */
int spk_gammas_exact_list(spk_ctx *ctx, int k, int32_t *out, int64_t n);
/* Per comparison column: pairs of the last spk_gammas whose level the filter took from the blocking
 * key instead of the rows -- a rule built by spk_key_build whose key includes the plain term
 * `l.c = r.c` on the raw columns the column was decoded from (spk_table_add_raw_utf8) emits only
 * pairs with equal, non-NULL values of c (the longest such run of the pair order; 0 when the
 * column holds an empty string, or was not built from raw columns). */
int spk_gammas_implied_pairs(spk_ctx *ctx, int64_t *out, int n);
/* Columns in the shape of the case_statements.py templates (NULL branch, then single-leaf tests
 * on the same two plain operands) are filtered from a packed per-row image of their fields
 * (spk_filter.hip); every other column by the general interpreter.  on = 1 (default): template
 * columns through the filter kernel; on = 0: every column through the interpreter; + 10: the second
 * blocking rule's pairs always read the table-ordered row image, + 20: always their rule's
 * view-ordered copy (default: the copy once the image outgrows the caches); + 100: leave every slow-list
 * launch to the settlement at the next synchronising call (by default only those of columns whose slow
 * lists were empty in the last call with the same pairs, tables and program).  All modes give
 * identical results (for testing).  spk_gammas_simple_count: how many columns the last spk_gammas
 * took as template columns. */
int spk_gammas_set_simple(spk_ctx *ctx, int on);
int spk_gammas_simple_count(spk_ctx *ctx, int *out);
/* Ordinal windows.  The reference joins and projects any number of pairs (blocking.py:95-160,
 * gammas.py:65-89); spk_gammas runs a pair set of more than ~2^31 pairs as consecutive windows of equal
 * size (the exact passes' work lists hold window-relative int32 ordinals), so one context takes any pair
 * count its device memory holds.  spk_gammas_set_window caps the window at `pairs` (0 = default, just under
 * 2^31; smaller windows give identical codes -- for testing); spk_gammas_windows: windows the last
 * spk_gammas ran. */
int spk_gammas_set_window(spk_ctx *ctx, int64_t pairs);
int spk_gammas_windows(spk_ctx *ctx, int64_t *out);
/* Two-stream split (an implementation choice, not a reference interface): with streams = 2 (default), a pair
 * set that fits one window and holds at least min_pairs pairs (default 2^22) runs as two windows of half the
 * pairs at once, the second on a stream of its own joined back before spk_gammas returns, so one window's
 * filter and the other's exact passes share the device.  streams = 1: one window on the context stream.
 * Identical codes either way (spk_gammas_windows reports 2 for a split call). */
int spk_gammas_set_streams(spk_ctx *ctx, int streams, int64_t min_pairs);
/* Graph replay (an implementation choice): a call whose program, pairs, tables, buffers, window layout and
 * slow-list decisions equal the previous call's records the pass's launches as a HIP graph; later such calls
 * (an EM run's iterations) replay it with one launch.  Off by default (on MI355X the replay measured slower than
 * direct launches); on = 0 enqueues every call directly.  Identical codes.
 * spk_gammas_graph_launches: replays so far on this context (diagnostics). */
int spk_gammas_set_graph(spk_ctx *ctx, int on);
int spk_gammas_graph_launches(spk_ctx *ctx, int64_t *out);
/* Levenshtein pass kernels (same codes in every mode; for A/B tests): 2 = lane refill (a lane that finishes its
 * cell takes the next one from its wave's queue) in the exact pass of free-text columns -- rows past 64 units on
 * both sides -- and one cell per lane elsewhere (default), 1 = lane refill in every exact pass (the 128-bit slow
 * pass stays one cell per lane), 0 = one cell per lane everywhere, 3 = as 2 without the character-bag decisions that precede a
 * refill pass over a free-text column (k_compact_lev: cells whose bag distance exceeds the cut take their level
 * there).  Modes 1 and 2 make those decisions too. */
int spk_gammas_set_lev_kernel(spk_ctx *ctx, int mode);
/* Filter field of a template Levenshtein column without free-text rows (same codes in both modes; for A/B tests):
 * 1 = the positional sketch (default) -- an 8-bit length and, for each half of the row, 30 buckets of 2-bit
 * saturating counts; the filter bounds the distance by the length gap, the whole-string bag distance of the summed
 * halves and a two-segment bag distance (a's first half against a prefix of b, its second against the rest), and
 * lists rows with equal fields for the exact pass (the field has no key); 0 = key, lengths and the whole-string
 * sketch.  A change of mode lays the row image out again at the next spk_gammas.  Free-text columns (rows past 64
 * units on both sides) keep the mode-0 field either way. */
int spk_gammas_set_lev_bound(spk_ctx *ctx, int mode);
/* Filter regions (workgroups) the last spk_gammas ran over the second rule's view-ordered image. */
int spk_gammas_view_regions(spk_ctx *ctx, int64_t *out);

/* ---- the jar's similarity UDFs as bulk device functions ---------------------------------
 * spk_jaro_winkler_sim replaces uk.gov.moj.dash.linkage.JaroWinklerSimilarity.call(String, String)
 * (commons-text 1.4 JaroWinklerDistance.apply, registered as `jaro_winkler_sim`, tests/test_spark.py:45);
 * spk_levenshtein replaces Spark's levenshtein(l, r) (case_statements.py:121).  n pairs of UTF-8 strings
 * (Arrow offsets, no NULLs), results in out[n] (host).  Same device code as the comparison kernel. */
int spk_jaro_winkler_sim(spk_ctx *ctx, int64_t n, const int64_t *l_offsets, const uint8_t *l_utf8,
                         const int64_t *r_offsets, const uint8_t *r_utf8, double *out);
int spk_levenshtein(spk_ctx *ctx, int64_t n, const int64_t *l_offsets, const uint8_t *l_utf8,
                    const int64_t *r_offsets, const uint8_t *r_utf8, double *out);
/* The jar's jaccard_sim and cosine_distance (SPK_OP_JACCARD / SPK_OP_COSINE above state the semantics), same
 * arguments.  spk_cosine_distance writes NaN for a pair with a blank text, where the reference throws. */
int spk_jaccard_sim(spk_ctx *ctx, int64_t n, const int64_t *l_offsets, const uint8_t *l_utf8,
                    const int64_t *r_offsets, const uint8_t *r_utf8, double *out);
int spk_cosine_distance(spk_ctx *ctx, int64_t n, const int64_t *l_offsets, const uint8_t *l_utf8,
                        const int64_t *r_offsets, const uint8_t *r_utf8, double *out);

/* ---- EM (replaces run_expectation_step + run_maximisation_step's aggregate,
 *      expectation_step.py:25-221, maximisation_step.py:41-90) ------------------ */
/* One EM iteration over this context's pairs in ONE launch: streams every pair's code into the
 * pattern histogram, and the workgroup that finishes last evaluates mp per pattern and the M-step
 * sums.  out_stats / m / u / lambda as spk_em_finalize.  For a single GPU (no exchange). */
int spk_em_iteration(spk_ctx *ctx, double lambda, double one_minus, const double *m, const double *u,
                     double *out_stats, int n_stats);
/* spk_em_iteration in two halves: _start enqueues the launch and the statistics readback (pinned host
 * memory) and returns; _wait returns the statistics.  In between the caller may enqueue the next
 * spk_gammas pass and compute the previous M-step on the host, so the device never waits for the host
 * (the reference's iterate loop, iterate.py:36-56, runs E, M, E, M ...: only the M-step of iteration i
 * must precede the E-step of i + 1).  If the codes the iteration read are corrected after spk_gammas
 * returned (work-list overflow, strings past the exact passes), the iteration is repeated before _wait
 * returns.  One iteration may be pending per context (SPK_E_STATE otherwise). */
int spk_em_iteration_start(spk_ctx *ctx, double lambda, double one_minus, const double *m, const double *u,
                           int n_stats);
int spk_em_iteration_wait(spk_ctx *ctx, double *out_stats, int n_stats);
/* Multi-GPU form of the same iteration: spk_em_histogram streams every pair's code once and writes
 * the pattern histogram (uint64 [n_patterns]) to d_hist, a DEVICE buffer (NULL = context-owned);
 * with a caller buffer it returns once the histogram is final.  Callers sharding pairs over GPUs
 * all-reduce it (exact integer sum), then spk_em_finalize. */
int spk_em_histogram(spk_ctx *ctx, uint64_t *d_hist);
/* Histogram kernel choice (same result): 1 = lane-private LDS counters when the pattern space fits, with an
 * agent-scope release fence before each last-arriver ticket (default: the memory model's own ordering; it
 * measured within 1 us of the unfenced form on MI355X, tools/ab_em_fence.py), 0 = wave-ballot aggregation
 * into one LDS histogram, 2 = as 1 without the fence (relies on gfx950 draining the row atomics before the
 * ticket).  For testing and measurement. */
int spk_em_set_lane_histogram(spk_ctx *ctx, int on);
/* The lane-private copies per pattern (64, 32, 16, 8 or 4) the E+M launch takes for the current pairs, pattern
 * space and histogram mode; 0 = the wave-ballot histogram + finalize launches.  For testing. */
int spk_em_lane_copies(spk_ctx *ctx, int *out);
/* E-step per pattern with the reference's literal arithmetic, then the M-step sums:
 * out_stats (host) = [Σmp, rows, non-null rows, Σ ln(λΠm + (1-λ)Πu), non-null ln rows] + per column k,
 * per level v in -1..L_k-1:
 * [rows, non-null rows, Σmp, Σ(1-mp)].  m/u are flattened [Σ L_k], already quantised as
 * `cast({p:.35f} as double)`; lambda/one_minus are `cast({λ} as double)`/`cast({1-λ} as double)`. */
int spk_em_finalize(spk_ctx *ctx, const uint64_t *d_hist, double lambda, double one_minus, const double *m,
                    const double *u, double *out_stats, int n_stats);
/* The multi-GPU iteration without host synchronisation: spk_em_histogram_async settles the last
 * spk_gammas (so every rank counts final codes and reduces exactly once) and enqueues the histogram into
 * d_hist; the caller enqueues its all-reduce on the context stream (spk_ctx_set_stream); then
 * spk_em_finalize_start enqueues the E-step + M-step sums and the statistics readback, and
 * spk_em_iteration_wait returns them. */
int spk_em_histogram_async(spk_ctx *ctx, uint64_t *d_hist);
int spk_em_finalize_start(spk_ctx *ctx, const uint64_t *d_hist, double lambda, double one_minus, const double *m,
                          const double *u, int n_stats);
/* Final E-step: match_probability per pair (NaN = NULL).  out_mp = host buffer for
 * [start, start+count), or NULL to keep the result on the device only. */
int spk_score(spk_ctx *ctx, double lambda, double one_minus, const double *m, const double *u, int64_t start,
              int64_t count, double *out_mp);

/* ---- selection of scored pairs (replaces df_e.filter(<predicate>) on the reference's Spark frames) ---- */
/* The reference hands back a Spark DataFrame, and its users keep the pairs they want with
 * df_e.filter("match_probability > 0.9") or a filter on gamma_* columns.  match_probability and every gamma are
 * functions of a pair's packed comparison code, so a conjunction over them is decided once per pattern (a keep
 * bitset); per pair the device does one bit lookup and a stable compaction (count per chunk of ordinals, scan,
 * emit), and only the survivors' ordinals, rows, codes are kept and later decoded. */
#define SPK_SEL_MP 0          /* match_probability under the parameters passed to spk_select (NaN = NULL) */
#define SPK_SEL_GAMMA 1       /* level of comparison column `col`, an integer in -1..L-1 (-1 is a value, not NULL) */
#define SPK_SEL_TF_MP 2       /* tf_adjusted_match_prob of the call's tables (NaN = NULL); spk_select_tf* only */
#define SPK_SEL_LT 0
#define SPK_SEL_LE 1
#define SPK_SEL_GT 2
#define SPK_SEL_GE 3
#define SPK_SEL_EQ 4
#define SPK_SEL_NE 5
#define SPK_SEL_IS_NULL 6
#define SPK_SEL_IS_NOT_NULL 7
#define SPK_SELECT_MAX_TERMS 8
typedef struct {
    int32_t field; /* SPK_SEL_MP / SPK_SEL_GAMMA / SPK_SEL_TF_MP */
    int32_t col;   /* comparison column (SPK_SEL_GAMMA) */
    int32_t op;    /* SPK_SEL_LT .. SPK_SEL_IS_NOT_NULL */
    int32_t pad;
    double value;  /* the literal the field is compared with */
} spk_select_term;
/* Keep the pairs for which every term is TRUE (SQL three-valued logic: a NULL match_probability fails every
 * comparison, != included; only IS NULL is true for it).  lambda / one_minus / m / u as for spk_score (m and u may
 * be NULL when no term reads match_probability; the survivors then carry no match_probability).  Needs comparison
 * codes (spk_gammas / spk_gammas_load), not pairs.  The survivors stay on the device, in ascending pair ordinal,
 * until the next spk_select or spk_select_release; a change of the pairs or the codes (spk_block*, spk_pairs_load,
 * spk_gammas, spk_gammas_load, a code correction at a synchronising call) makes them stale.  A failing call leaves
 * no selection.  Does not touch the scores of spk_score or any term-frequency state. */
int spk_select(spk_ctx *ctx, double lambda, double one_minus, const double *m, const double *u, int n_terms,
               const spk_select_term *terms, int64_t *out_n_selected);
/* Survivors [start, start + count) of the last spk_select (any output may be NULL): pair ordinal, the pair's rows
 * (SPK_E_STATE without a pair set: a loaded gamma table), the int8 levels [count x K] decoded from the survivors'
 * codes, and match_probability (SPK_E_STATE when spk_select got no m / u).  SPK_E_STATE for a stale selection. */
int spk_select_copy(spk_ctx *ctx, int64_t start, int64_t count, int64_t *out_ordinal, int32_t *out_l,
                    int32_t *out_r, int8_t *out_gammas, double *out_mp);
/* The last spk_select: survivors (-1: none, released or replaced by a failed call), and with timing on
 * (spk_ctx_enable_timing) the device milliseconds of its kernels (pattern table and bitset, count pass and scan,
 * emit pass; the host round trip between them is not in it), -1 otherwise. */
int spk_select_info(spk_ctx *ctx, int64_t *out_n_selected, double *out_ms);
int spk_select_release(spk_ctx *ctx);
/* The same with terms on tf_adjusted_match_prob = bayes(mp, adj_1, ..., adj_n) (term_frequencies.py:98-117; replaces
 * filtering the frame make_adjustment_for_term_frequencies returns).  That score depends on the pair's code (through
 * mp) and on its two rows (through the tf value ids), so it is decided per pair, as a cascade: the SPK_SEL_MP and
 * SPK_SEL_GAMMA terms go through the pattern bitset as in spk_select, and only the pairs whose pattern passes them
 * gather their value ids and table entries and evaluate the SPK_SEL_TF_MP terms (NaN = NULL, three-valued as above).
 * The value compared and returned is the one spk_tf_apply* gives for the pair under the same tables and the mp of
 * lambda / m / u, bit for bit (one shared device function).  Value ids and tables as for spk_tf_apply (host ids) and
 * spk_tf_apply_columns (device dictionary ids); they are used during the call only.  m and u are required, n_tf_cols
 * is 1..8, terms may mix all three fields (at most SPK_SELECT_MAX_TERMS in total; none with field SPK_SEL_TF_MP is
 * legal and still yields the tf outputs), and the context needs a pair set with rows (SPK_E_STATE for a loaded gamma
 * table).  The result is the context's one selection, as after spk_select (spk_select_copy, spk_select_info,
 * spk_select_release and spk_components work on it), which also holds the survivors' tf_adjusted_match_prob and
 * adjustments.  Nothing of P elements in fp64 is stored: the count pass keeps one keep bit per pair (P / 8 bytes)
 * for the emit pass and frees it.  Reads and writes nothing of spk_score's scores, the device-resident tf results of
 * spk_tf_apply*, the tf sums' state or the EM state.  A failing call leaves no selection. */
int spk_select_tf(spk_ctx *ctx, double lambda, double one_minus, const double *m, const double *u, int n_tf_cols,
                  const int64_t *const *ids_side0, const int64_t *const *ids_side1, const double *const *adj_tables,
                  const int64_t *table_sizes, int n_terms, const spk_select_term *terms, int64_t *out_n_selected);
int spk_select_tf_columns(spk_ctx *ctx, double lambda, double one_minus, const double *m, const double *u,
                          int n_tf_cols, const int32_t *cols, const double *const *adj_tables,
                          const int64_t *table_sizes, int n_terms, const spk_select_term *terms,
                          int64_t *out_n_selected);
/* Survivors [start, start + count) of the last spk_select_tf*: tf_adjusted_match_prob and the adjustments
 * (either may be NULL).  SPK_E_STATE after a plain spk_select, without a selection, or for a stale one. */
int spk_select_copy_tf(spk_ctx *ctx, int64_t start, int64_t count, double *out_tf_mp,
                       double *out_adj /* [count x n_tf_cols] or NULL */);

/* ---- a stratified random sample of the scored pairs (replaces df_e.toPandas() followed by a pandas
 *      groupby(score band).sample(k), the clerical-review sample the reference's users label by hand) ---- */
#define SPK_SAMPLE_MAX_STRATA 64
/* Keeps, per score band, the quota[b] pairs with the smallest random keys.  The result is this set, whatever the
 * launch shape:
 *   mix(x):       x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB; x ^= x >> 31
 *   key(seed, p): mix(mix(seed) + 0x9E3779B97F4A7C15 * (p + 1)) in 64-bit wrap-around arithmetic, p the pair's ordinal
 *                 (as spk_select_copy reports it); a bijection of p, so no two pairs share a key
 *   strata:       n_strata + 1 finite, strictly ascending edges, 1 <= n_strata <= SPK_SAMPLE_MAX_STRATA; a pair whose
 *                 match_probability x (under lambda / m / u, as spk_score) is not NULL and lies in
 *                 [edges[0], edges[n_strata]] is in the stratum b with edges[b] <= x < edges[b + 1], the last stratum
 *                 also taking x == edges[n_strata]; any other pair is in no stratum
 *   eligible:     in a stratum, and every term TRUE (spk_select's conjunction and three-valued logic; fields SPK_SEL_MP
 *                 and SPK_SEL_GAMMA; n_terms = 0: all)
 *   kept:         in stratum b the min(quota[b], population[b]) eligible pairs with the smallest keys
 * So a larger quota under the same seed keeps a superset, and a stratum with population <= quota is kept whole.
 * This is a selecting call: it drops the previous selection first, and on success the context's one selection holds
 * the kept pairs in ascending ordinal (rows when the pair set has them, codes, the mp table); spk_select_copy,
 * spk_select_info, spk_select_release, spk_select_best, spk_components* and spk_label_scores_selection work on it
 * unchanged, and it goes stale as spk_select's does.  m and u are required.  The thresholds are found by a radix select
 * over the keys, 8 passes of 8 bits over the codes with one histogram per stratum, then spk_select's count, scan and
 * emit: nothing of P elements is allocated but the chunk counts.  SPK_E_INVALID: edges not finite or not strictly
 * ascending, n_strata out of range, a negative quota, an unknown field (SPK_SEL_TF_MP included) or operator, and
 * spk_select's argument errors.  SPK_E_STATE: no gammas.  A failing call leaves no selection.  Does not touch the
 * scores of spk_score, tf state or EM state. */
int spk_select_sample(spk_ctx *ctx, double lambda, double one_minus, const double *m, const double *u, int n_terms,
                      const spk_select_term *terms, int n_strata, const double *edges /* [n_strata + 1] */,
                      const int64_t *quota /* [n_strata] */, uint64_t seed, int64_t *out_n_selected);
/* The last spk_select_sample: its strata (-1: none yet, or the last call failed; nothing else is written then), per
 * stratum the eligible pairs and the pairs kept (the first n_strata entries; either may be NULL), and with timing on
 * (spk_ctx_enable_timing) the device milliseconds of its launches (pattern stage, histogram passes and digit picks,
 * count pass and scan, emit pass; the host round trip between them is not in it), -1 otherwise. */
int spk_select_sample_info(spk_ctx *ctx, int *out_n_strata, int64_t *out_population /* [n_strata] */,
                           int64_t *out_kept /* [n_strata] */, double *out_ms);

/* ---- best match per record (replaces the window query the reference's users run over the frame
 *      expectation_step.py returns: row_number() over (partition by unique_id_l order by match_probability desc) = 1,
 *      often once per side and then joined, to link each record to its best candidate) ---- */
/* Narrows the context's selection to the best pair per record.  S = the survivors whose score is not NULL (NaN); the
 * score is `field`: SPK_SEL_MP (the selection's own match_probability) or SPK_SEL_TF_MP (its tf_adjusted_match_prob).
 * Pair a beats pair b iff score(a) > score(b), or the scores are equal as doubles and ordinal(a) < ordinal(b): a
 * strict total order (Spark's row_number leaves ties unspecified; here the ordinal decides, since thousands of pairs
 * share one comparison pattern and so one score).  A record is a row of an input table; link_only never identifies a
 * left with a right record, dedupe_only and link_and_dedupe index table 0 on both sides. */
#define SPK_BEST_L 0          /* kept: the pair beats every other pair of S with the same left record */
#define SPK_BEST_R 1          /* the same by right record */
#define SPK_BEST_EITHER 2     /* best[x] = the pair that beats all pairs of S touching record x on either side; kept iff
                                 it is best[l] or best[r] */
#define SPK_BEST_MUTUAL 3     /* kept iff it is best[l] and best[r]: every record is then in at most one kept pair */
/* keep_ties = 0: as above.  keep_ties = 1: every pair whose score equals its group's maximum is a best pair of the
 * group (no ordinal tie-break), combined per mode in the same way.  A pair with a NULL score is never kept and never
 * beats anything.  The kept pairs stay in ascending pair ordinal and REPLACE the context's selection:
 * spk_select_copy, spk_select_copy_tf, spk_select_info (whose milliseconds stay those of the selecting call) and
 * spk_components work on them unchanged, and their buffers, sized to the kept count, count under [6] of
 * spk_ctx_memory; the per-record arrays of the passes are freed before the call returns.  An empty selection is
 * legal and keeps 0.  SPK_E_INVALID: unknown field, mode or keep_ties.  SPK_E_STATE: no selection; a stale one; one
 * without pair rows (a loaded gamma table); SPK_SEL_MP on a selection made without m / u; SPK_SEL_TF_MP on one not
 * made by spk_select_tf*.  A failing call leaves no selection.  The result does not depend on launch shape or on the
 * arrival order of the atomics.  Reads the selection and the tables' row counts only: the scores of spk_score, tf
 * state, EM state and component labels are not touched. */
int spk_select_best(spk_ctx *ctx, int field /* SPK_SEL_MP | SPK_SEL_TF_MP */, int mode, int keep_ties,
                    int64_t *out_n_kept);
/* The last spk_select_best: survivors before it and pairs kept (-1 each: none yet, or the last call failed), and
 * with timing on (spk_ctx_enable_timing) the device milliseconds of its launches (group maxima, first index, keep
 * flags and scan, emit; the host round trip between them is not in it), -1 otherwise. */
int spk_select_best_info(spk_ctx *ctx, int64_t *out_n_before, int64_t *out_n_kept, double *out_ms);

/* ---- the first k pairs in score order (replaces df_e.orderBy("match_probability", ascending=False).limit(k) on the
 *      frame expectation_step.py returns, which here would be toPandas() and a host sort of every pair) ---- */
#define SPK_TOP_FIRST 0   /* frame order: the first k by ordinal */
#define SPK_TOP_ASC   1
#define SPK_TOP_DESC  2
/* The result is this set, whatever the algorithm, chunking or launch shape.  The score is a double and NaN means NULL.
 * Values are ordered as Spark orders them by default: NULL is smaller than every number, numbers compare as doubles
 * (-0.0 equals +0.0).  SPK_TOP_ASC: pair a comes before pair b iff score(a) < score(b), or the scores are equal (two
 * NULLs are) and ordinal(a) < ordinal(b); SPK_TOP_DESC: the same with score(a) > score(b), so NULLs come first
 * ascending and last descending, and the ordinal (as spk_select_copy reports it) breaks ties in both directions: a
 * strict total order.  SPK_TOP_FIRST: ascending ordinal alone.  Kept: the first min(k, eligible) eligible pairs in
 * that order; k = 0 keeps none.  When 0 < k < eligible under a score order, the cut is the score of the k-th pair,
 * `tied` the eligible pairs with that score (the eligible NULL pairs when it is NULL) and `tied_kept` how many of them
 * are kept, the ones with the smallest ordinals; otherwise there is no cut and both are 0.
 *
 * spk_select_top is a selecting call, called like spk_select_sample: eligible = every term TRUE (spk_select's
 * conjunction and three-valued logic; fields SPK_SEL_MP and SPK_SEL_GAMMA; n_terms = 0: all), the score is
 * match_probability under lambda / m / u (as spk_score).  m / u may be NULL only with SPK_TOP_FIRST and no SPK_SEL_MP
 * term.  It drops the previous selection first, and on success the context's one selection holds the kept pairs in
 * ascending ordinal (not in score order); spk_select_copy, spk_select_info, spk_select_release, spk_select_best,
 * spk_components* and spk_label_scores_selection work on it unchanged, and it goes stale as spk_select's does.  The
 * score is a function of the pattern, so the cut is found on the pattern table: one pass over the codes counts the
 * pairs per pattern, a weighted radix select over the eligible patterns' score keys (8 passes of 8 bits over
 * n_patterns entries) finds the cut score and how many pairs at the cut are kept, one byte per pattern says above the
 * cut / at the cut / out, and spk_select's count, scan and emit run with two counts per chunk: a pair at the cut is
 * emitted iff fewer than tied_kept pairs at the cut precede it.  Nothing of P elements is allocated but the chunk
 * counts; no workgroup waits for another, every loop has a fixed bound and the histograms are integer sums, so nothing
 * depends on the order in which atomics arrive.  SPK_E_INVALID: unknown order, negative k, a score order without m / u,
 * an unknown field (SPK_SEL_TF_MP included) or operator, and spk_select's argument errors.  SPK_E_STATE: no gammas.  A
 * failing call leaves no selection.  Does not touch the scores of spk_score, tf state, EM state or component labels. */
int spk_select_top(spk_ctx *ctx, double lambda, double one_minus, const double *m, const double *u, int n_terms,
                   const spk_select_term *terms, int order, int64_t k, int64_t *out_n_selected);
/* Narrows the context's selection, as spk_select_best does, to its first k survivors under `order`; eligible = every
 * survivor, the score is the selection's own stored one: SPK_SEL_MP (its match_probability) or SPK_SEL_TF_MP (its
 * tf_adjusted_match_prob); `field` is ignored for SPK_TOP_FIRST.  The kept pairs stay in ascending pair ordinal and
 * REPLACE the selection: spk_select_copy, spk_select_copy_tf, spk_select_info (whose milliseconds stay those of the
 * selecting call) and spk_components* work on them unchanged.  The cut comes from a radix select over an
 * order-preserving 64-bit key of the survivors' scores, most significant byte first, one histogram and one pick launch
 * per pass, then the two-count count, scan and emit over the survivors.  An empty selection is legal and keeps 0.
 * SPK_E_INVALID: unknown order or field, negative k.  SPK_E_STATE: no selection; a stale one; SPK_SEL_MP on a selection
 * made without m / u; SPK_SEL_TF_MP on one not made by spk_select_tf*.  A failing call leaves no selection.  Does not
 * touch the scores of spk_score, tf state, EM state or component labels. */
int spk_select_top_of(spk_ctx *ctx, int field /* SPK_SEL_MP | SPK_SEL_TF_MP; ignored for SPK_TOP_FIRST */, int order,
                      int64_t k, int64_t *out_n_kept);
/* The last spk_select_top / spk_select_top_of: eligible pairs, pairs kept, pairs at the cut and how many of those are
 * kept (-1 each: none yet, or the last call failed), the cut score (NaN when there is no cut, and when the cut is NULL:
 * out_tied is 0 in the first case and positive in the second), and with timing on (spk_ctx_enable_timing) the device
 * milliseconds of its launches (pattern stage and histogram, digit passes and picks, count pass and scans, emit pass;
 * the host round trip between them is not in it), -1 otherwise. */
int spk_select_top_info(spk_ctx *ctx, int64_t *out_eligible, int64_t *out_kept, double *out_cut_score,
                        int64_t *out_tied, int64_t *out_tied_kept, double *out_ms);

/* ---- connected components of the kept pairs (replaces handing df_e.filter(...) to GraphFrames'
 *      connectedComponents; later reference releases: cluster_pairwise_predictions_at_threshold) ---- */
/* label[v] = the smallest node id of v's component in the graph whose edges are the survivors of the last spk_select;
 * a node without edges keeps label[v] = v.  Node ids are INPUT positions, not device rows (spk_cluster permutes
 * those): dedupe_only and link_and_dedupe have the n0 rows of table 0 as nodes (the latter: the vertical
 * concatenation, left rows first); link_only has n0 + n1 nodes, a right row r being node n0 + its input position.
 * Min-label hooking with pointer jumping, one host-read "changed" word per round; the result does not depend on
 * edge order, launch shape or the arrival order of the atomics.  out_n_clusters counts the nodes with label[v] == v
 * (singletons included); out_rounds the rounds run, the last quiet one included (0 without edges).  SPK_E_STATE
 * without a selection, with a stale one, or with one that has no pair rows (a loaded gamma table); SPK_E_LIMIT past
 * 2^32 - 1 nodes or when the round cap (256) is reached.  The labels stay on the device until the next
 * spk_components*, spk_components_release, or a change of the tables (spk_table_create, spk_cluster); they do not
 * depend on the selection, the codes or the pairs once built, and a failing call leaves none.  Reads the selection
 * and the tables' permutations only: scores, tf and EM state are not touched. */
int spk_components(spk_ctx *ctx, int64_t *out_n_nodes, int64_t *out_n_clusters, int *out_rounds);
/* The same over host edges u[i] -- v[i] with ids in [0, n_nodes): any graph, no tables needed (the building block
 * for merging the clusters of several shards).  Self-loops, repeated edges and both orientations are legal; an id
 * >= n_nodes is SPK_E_INVALID (found on the device in the first pass, no label is read or written for that edge). */
int spk_components_edges(spk_ctx *ctx, int64_t n_nodes, int64_t n_edges, const uint32_t *u, const uint32_t *v,
                         int64_t *out_n_clusters, int *out_rounds);
/* Labels of nodes [start, start + count) of the last spk_components* (SPK_E_STATE: none). */
int spk_components_copy(spk_ctx *ctx, int64_t start, int64_t count, uint32_t *out_label);
/* The last spk_components*: nodes and edges (-1: none, released or replaced by a failed call), rounds, and with
 * timing on (spk_ctx_enable_timing) the device milliseconds of its kernels (edge build, every round's hook and jump
 * launches, the cluster count; the host round trip after each round is not in it), -1 otherwise. */
int spk_components_info(spk_ctx *ctx, int64_t *out_n_nodes, int64_t *out_n_edges, int *out_rounds, double *out_ms);
int spk_components_release(spk_ctx *ctx);
/* The same labels into device memory (the source of an all-gather over the ranks): a device-to-device copy on the
 * context's stream, complete when the call returns. */
int spk_components_copy_device(spk_ctx *ctx, int64_t start, int64_t count, uint32_t *d_out_label);

/* ---- the clusters of a multi-GPU job: the ranks' components merged on the device ---- */
#define SPK_COMPONENTS_MAX_PEERS 64 /* label arrays per merge call; call again for more */
/* Brings the labels of the last spk_components*, in place, to the smallest-id labels of the union of their graph with
 * n_peers other graphs over the same node ids.  Graph p is named by row p of peer_labels (n_peers rows of `stride`
 * uint32 each, stride >= n_nodes, entries past n_nodes never read): any array with peer[v] <= v whose edges
 * (v, peer[v]) span that graph's components, such as another rank's final labels.  on_device = 0: a host pointer,
 * uploaded for the call (n_peers * stride * 4 bytes, freed before it returns); otherwise a device pointer on the
 * context's device, read in place, whose writes must have completed.  No edge list is built: the rounds of
 * spk_components run with a node launch that also hooks, per node v and peer p, (v, peer_p[v]).  The first round checks
 * every peer entry before it indexes anything with it: an entry > its own index (hence any entry >= n_nodes) is
 * SPK_E_INVALID, and like every failure past the argument checks it leaves no components.  out_n_clusters is the
 * merged count, out_rounds the rounds of this call (the quiet one included, >= 1); spk_components_info then reports
 * the sum of the rounds (and milliseconds) so far and, unchanged, the nodes and this graph's own edges.  May be called
 * repeatedly, each call merging more graphs in (a ring, or a gather in groups, bounds the memory of one call).
 * SPK_E_INVALID: n_peers outside 1..SPK_COMPONENTS_MAX_PEERS, NULL peer_labels, stride < n_nodes.  SPK_E_STATE: no
 * components.  SPK_E_LIMIT: the round cap.  The selection, scores, tf and EM state and the sweep are not touched. */
int spk_components_merge(spk_ctx *ctx, int n_peers, const uint32_t *peer_labels, int64_t stride, int on_device,
                         int64_t *out_n_clusters, int *out_rounds);

/* ---- clusters at several thresholds in one pass, and their metrics (no counterpart in the reference release, whose
 *      users loop connectedComponents over df_e.filter(...) and groupBy the result; later releases:
 *      cluster_pairwise_predictions_at_multiple_thresholds, compute_graph_metrics) ---- */
#define SPK_SEL_ALL (-1)            /* every survivor of the selection, whatever its score */
#define SPK_SWEEP_MAX_LEVELS 32
/* L = n_thresholds levels of labels over the survivors of the last spk_select*: level k's edges are the survivors
 * whose score -- `field`: SPK_SEL_MP (the selection's match_probability) or SPK_SEL_TF_MP (its
 * tf_adjusted_match_prob) -- is > thresholds[k], the strict test of SPK_SEL_GT on the same doubles; a NaN score is in
 * no level.  field SPK_SEL_ALL: n_thresholds must be 0, L = 1 and every survivor is an edge.  thresholds are strictly
 * descending and not NaN (+-inf are legal), 1..SPK_SWEEP_MAX_LEVELS of them: anything else is SPK_E_INVALID.
 * label_k[v] is the smallest node id of v's component at level k, node ids as spk_components defines them, so level
 * k equals, bit for bit, what spk_select(score > thresholds[k]) followed by spk_components gives; it does not depend
 * on the algorithm, the edge order, the launch shape or the arrival order of the atomics.  The edge sets are nested,
 * so each level starts from the previous level's labels and hooks only the edges that are new at it (plus, per node,
 * the edge to its previous label).  out_n_edges[k] is cumulative (the edges of level k), out_n_clusters[k] counts the
 * nodes with label_k[v] == v, out_rounds[k] the rounds level k ran (0: no new edge).  SPK_E_STATE: the cases of
 * spk_components; SPK_SEL_MP on a selection made without m / u; SPK_SEL_TF_MP on one not made by spk_select_tf*.
 * SPK_E_LIMIT: as spk_components, per level.  The sweep is a value of its own: it holds L x n_nodes labels and the
 * edges bucketed by level (8 bytes each, kept for spk_cluster_metrics), counted under [6] of spk_ctx_memory; it
 * needs the selection only while it is built, and stays until the next spk_components_sweep*, its release, or a
 * change of the tables (spk_table_create, spk_cluster).  spk_components* and the sweep do not disturb each other's
 * result; a failing call leaves no sweep.  Reads the selection and the tables' permutations only: scores, tf state,
 * EM state, the selection and the labels of spk_components are not touched. */
int spk_components_sweep(spk_ctx *ctx, int field /* SPK_SEL_MP | SPK_SEL_TF_MP | SPK_SEL_ALL */, int n_thresholds,
                         const double *thresholds, int64_t *out_n_nodes, int64_t *out_n_edges /* [L] */,
                         int64_t *out_n_clusters /* [L] */, int *out_rounds /* [L] */);
/* The same over host edges u[i] -- v[i] with ids in [0, n_nodes) and a score each (n_thresholds = 0: as SPK_SEL_ALL,
 * score may be NULL, a NaN score is then an edge too).  Self-loops, repeated edges and both orientations are legal; an
 * id >= n_nodes in an edge of some level is SPK_E_INVALID. */
int spk_components_sweep_edges(spk_ctx *ctx, int64_t n_nodes, int64_t n_edges, const uint32_t *u, const uint32_t *v,
                               const double *score, int n_thresholds, const double *thresholds,
                               int64_t *out_n_edges /* [L] */, int64_t *out_n_clusters /* [L] */,
                               int *out_rounds /* [L] */);
/* Labels of nodes [start, start + count) at `level` of the last sweep (SPK_E_STATE: none; SPK_E_INVALID: a level or
 * range outside it). */
int spk_components_sweep_copy(spk_ctx *ctx, int level, int64_t start, int64_t count, uint32_t *out_label);
/* The last sweep: levels, nodes, edges of its last level (-1 each: none), and with timing on the device milliseconds
 * of its kernels (edge build, level assignment and bucketing, every level's label copy, rounds and cluster count; the
 * host round trip after each round is not in it), -1 otherwise. */
int spk_components_sweep_info(spk_ctx *ctx, int *out_levels, int64_t *out_n_nodes, int64_t *out_n_edges, double *out_ms);
int spk_components_sweep_release(spk_ctx *ctx);
/* The labels of one level into device memory, as spk_components_copy_device. */
int spk_components_sweep_copy_device(spk_ctx *ctx, int level, int64_t start, int64_t count, uint32_t *d_out_label);
/* spk_components_merge on level `level` of the current sweep, with its arguments, checks and failure rule (a failure
 * past the argument checks leaves no sweep).  Level k of every rank merged gives level k of the whole pair set, and
 * unions of nested sets are nested, so the levels are merged one at a time and independently: n_peers * stride labels
 * are held per call, not L times that.  out_n_clusters replaces the level's count, out_rounds (this call's) is added
 * to the level's rounds.  A sweep with a merged level is marked: its edges are one shard's, so spk_cluster_metrics on
 * it is SPK_E_STATE (and the last metrics are dropped); spk_cluster_agreement, which reads labels only, keeps working.
 * SPK_E_INVALID also for a level outside the sweep; SPK_E_STATE: no sweep. */
int spk_components_sweep_merge(spk_ctx *ctx, int level, int n_peers, const uint32_t *peer_labels, int64_t stride,
                               int on_device, int64_t *out_n_clusters, int *out_rounds);
/* Which edges a level's rounds hook (both give the same labels; for A/B runs): 0 (default) the edges that are new at
 * the level, plus for every node the edge to its label at the previous level; 1 every edge of the level. */
int spk_components_sweep_set_mode(spk_ctx *ctx, int mode);

/* Metrics of one level of the last sweep, integer counting on the device, exact and repeatable.  degree[v] counts
 * the level's edges incident to v: an edge u -- v adds 1 to each end, a self-loop of host edges 2, a repeated edge
 * counts each time (a selection has neither).  The per-cluster arrays are indexed by node id, meaningful at the roots
 * (label[v] == v) and 0 elsewhere: size = nodes of the cluster, degree_sum = the sum of its degrees (twice its
 * edges), max_degree = its largest degree.  out3 = clusters of >= 2 nodes, nodes in them, the largest cluster's
 * nodes (0 without nodes).  The arrays (20 bytes per node, under [6] of spk_ctx_memory) describe one level at a time:
 * they are recomputed by every call and freed with the sweep.  SPK_E_STATE without a sweep or on one with a merged
 * level (spk_components_sweep_merge), SPK_E_INVALID for a level outside it. */
int spk_cluster_metrics(spk_ctx *ctx, int level, int64_t *out3);
/* Nodes [start, start + count) of the last spk_cluster_metrics; any out may be NULL. */
int spk_cluster_metrics_copy(spk_ctx *ctx, int64_t start, int64_t count, uint32_t *out_degree, uint32_t *out_size,
                             uint64_t *out_degree_sum, uint32_t *out_max_degree);
/* The edge pass of spk_cluster_metrics (both give the same counts; for A/B runs): 1 (default) the lanes of a wave that
 * share the first lane's end are counted in the wave and issue one add; 0 one add per edge end. */
int spk_cluster_metrics_set_mode(spk_ctx *ctx, int mode);
/* The level of the last spk_cluster_metrics (-1: none) and, with timing on, the milliseconds of its kernels. */
int spk_cluster_metrics_info(spk_ctx *ctx, int *out_level, double *out_ms);

/* Bridges and 2-edge-connected cores of one level of the last sweep (later releases: the edge metric is_bridge of
 * compute_graph_metrics).  The level's graph is its cumulative edge set as stored, over n_nodes nodes.  An edge with
 * u != v is a bridge iff deleting that one stored edge leaves u and v in different components: a self-loop never is, and
 * an edge stored twice never is, in either orientation (host edge lists allow repeats, a selection has none).  For a
 * bridge (u, v), side_u and side_v are the node counts of the two parts its cluster falls into without it (their sum is
 * the cluster's size).  core[v] is the smallest node id of v's component once every bridge is cut -- its
 * 2-edge-connected component; a node without edges keeps core[v] = v.  Bridges come in the orientation in which the edge
 * is stored (a selection: u the left row's node, v the right's), ascending by (u, v).  Exact integers that depend on
 * neither the spanning tree chosen nor the arrival order of the atomics: two calls give the same bytes.
 * out4 = bridges, cores (nodes with core[v] == v), nodes of the largest core, depth of the deepest breadth-first tree
 * (rooted at each cluster's smallest id).  The forest takes depth + 1 host-driven rounds over the level's edges (0
 * without edges); a tree deeper than 4095 is SPK_E_LIMIT (a chain of thousands of records).  The result (16 bytes per
 * bridge, 4 per node, under [6] of spk_ctx_memory) is a value of its own: a call that fails past its argument checks
 * leaves none, and the sweep as it was; it is replaced by the next spk_cluster_bridges and dropped with the sweep (and
 * by spk_components_sweep_merge); it and the arrays of spk_cluster_metrics do not disturb each other.  SPK_E_STATE without
 * a sweep or on one with a merged level (its edges are one shard's), SPK_E_INVALID for a level outside it.  Reads the
 * sweep only: its labels and metrics, the labels of spk_components, the selection, scores, tf and EM state are
 * untouched. */
int spk_cluster_bridges(spk_ctx *ctx, int level, int64_t *out4);
/* Bridges [start, start + count) of the last spk_cluster_bridges, in (u, v) order; any out may be NULL.  SPK_E_STATE:
 * none; SPK_E_INVALID: a range outside them. */
int spk_cluster_bridges_copy(spk_ctx *ctx, int64_t start, int64_t count, uint32_t *out_u, uint32_t *out_v,
                             uint32_t *out_side_u, uint32_t *out_side_v);
/* core[v] of nodes [start, start + count) of the last spk_cluster_bridges. */
int spk_cluster_bridges_cores_copy(spk_ctx *ctx, int64_t start, int64_t count, uint32_t *out_core);
/* The level of the last spk_cluster_bridges (-1: none), its forest rounds, and with timing on the device milliseconds
 * of its kernels (the host round trip after each round is not in it), -1 otherwise. */
int spk_cluster_bridges_info(spk_ctx *ctx, int *out_level, int *out_rounds, double *out_ms);

/* ---- clusters against labels (no counterpart in the reference release) ---- */
#define SPK_AGREE_FIELDS 10
/* Every level of the current sweep (spk_components_sweep / _sweep_edges) against one truth id per node.
 * ids: n_nodes values in node order, negative = NULL, an id >= 2^31 is SPK_E_INVALID (as spk_label_histogram).
 * n_left in [0, n_nodes]; read only when cross_only != 0.  out: levels x SPK_AGREE_FIELDS, level-major.
 * A node is labelled iff its id is >= 0; a counted pair is an unordered pair of distinct labelled nodes, under
 * cross_only only one with a node < n_left and a node >= n_left.  Per level, with c the level's labels and g the ids:
 *   [0] records_labelled    labelled nodes
 *   [1] clusters_labelled   clusters holding a labelled node
 *   [2] entities            distinct ids
 *   [3] predicted_pairs     counted pairs with c[u] == c[v]
 *   [4] true_pairs          counted pairs with g[u] == g[v]
 *   [5] tp                  counted pairs with both
 *   [6] clusters_mixed      clusters whose labelled nodes carry two or more ids
 *   [7] entities_split      ids whose nodes lie in two or more clusters
 *   [8] entities_recovered  ids whose nodes all lie in one cluster that holds no labelled node of another id
 *   [9] pairs_total         all counted pairs: C(M, 2), or M_left * M_right under cross_only
 * [0], [2], [4] and [9] do not depend on the level and are filled in every row.  Exact integers from sorted keys,
 * independent of launch shape and of the arrival order of the atomics: two calls give the same bytes.
 * SPK_E_STATE: no sweep.  SPK_E_INVALID: NULL ids (with n_nodes > 0), NULL out, n_left out of range under cross_only,
 * an id >= 2^31 (found on the device before any id is used).  SPK_E_LIMIT: more than 2^31 nodes.
 * Reads the sweep's labels and writes nothing of the context but the two numbers of spk_cluster_agreement_info (a
 * failing call leaves those as they were): the sweep, its metrics, the labels of spk_components, the selection, scores,
 * tf and EM state are untouched, and every device buffer of the call is freed before it returns. */
int spk_cluster_agreement(spk_ctx *ctx, const int64_t *ids, int64_t n_left, int cross_only, int64_t *out);
/* The last successful spk_cluster_agreement: its levels (-1: none yet) and, with timing on, the device milliseconds
 * of all its launches (the upload and the read-backs are not in it), -1.0 otherwise. */
int spk_cluster_agreement_info(spk_ctx *ctx, int *out_levels, double *out_ms);   /* -1 / -1.0: none yet / timing off */

/* ---- pairs against labels (no counterpart in the reference release; later releases:
 *      truth_space_table_from_labels_column, estimate_m_from_label_column) ---- */
#define SPK_LABEL_NON_MATCH 0   /* both labels non-NULL and different */
#define SPK_LABEL_MATCH     1   /* both labels non-NULL and equal */
#define SPK_LABEL_UNKNOWN   2   /* either label NULL */
#define SPK_LABEL_STATES    3
/* One pass over the context's pairs that counts them per (truth state, comparison pattern):
 * out_counts[s * n_patterns + code] = pairs with state s and packed code `code`; the three states sum to bin `code`
 * of spk_em_histogram.  match_probability is a function of the code alone, so these counts hold the exact confusion
 * matrix at every threshold and the supervised m / u / lambda estimate.  ids_side* are one label id per record, in
 * device row order (as for spk_tf_accumulate), one id space for both sides; any negative id is NULL.  ids_side1 may
 * be NULL when the pairs' right rows index table 0 (dedupe_only, link_and_dedupe).  The ids are narrowed to 32 bits
 * on the device (half the gathered footprint); an id >= 2^31 is SPK_E_INVALID.  With m and u, out_pattern_mp[code]
 * is the match_probability of the pattern under lambda / one_minus / m / u as for spk_score, by the same device
 * function, bit for bit; without them it must be NULL.  The counts are integers: they do not depend on launch shape or
 * on the arrival order of the atomics, and ranks holding shards of the pairs sum them.
 * SPK_E_STATE: no comparison codes, or no pair rows (a loaded gamma table).  SPK_E_INVALID: NULL ids_side0; NULL
 * ids_side1 under link_only; NULL out_counts; out_pattern_mp without m / u.  SPK_E_LIMIT: 3 * n_patterns > 2^30.
 * Reads the pairs and the codes only: no selection, score, tf, EM or component state is touched, and the call's
 * device buffers are freed before it returns. */
int spk_label_histogram(spk_ctx *ctx, const int64_t *ids_side0, const int64_t *ids_side1,
                        double lambda, double one_minus, const double *m, const double *u,
                        uint64_t *out_counts   /* host [SPK_LABEL_STATES x n_patterns], state-major */,
                        double *out_pattern_mp /* host [n_patterns] or NULL */);
/* The last spk_label_histogram: pairs counted (-1: none yet, or the last call failed), and with timing on
 * (spk_ctx_enable_timing) the device milliseconds of its launches (id narrowing, pattern table, counter clear and
 * the histogram; the uploads and read-backs are not in it), -1 otherwise. */
int spk_label_info(spk_ctx *ctx, int64_t *out_pairs, double *out_ms);

/* ---- pairs against a table of labelled pairs (later releases: truth_space_table_from_labels_table,
 *      prediction_errors_from_labels_table, estimate_m_from_pairwise_labels; replaces taking every scored pair to the
 *      host and merging it with the labels there) ---- */
/* spk_label_histogram's counts with the truth state of a candidate pair looked up in a set of n_labels labelled pairs,
 * e.g. a clerical-review sample: MATCH and NON_MATCH hold the labelled candidate pairs, UNKNOWN the candidate pairs
 * without a label, and the three rows sum to spk_em_histogram bin for bin.  rows_l / rows_r are device rows (as
 * spk_pairs_copy gives them), is_match is 0 or 1.  n_labels = 0 is legal: every pair is UNKNOWN.
 * The set is a hash table built on the device for the call:
 *   - open addressing with linear probing (slot + 1, wrapping), one 64-bit word per slot, an empty slot all ones;
 *   - capacity = the smallest power of two >= 2 * n_labels, and at least 64;
 *   - key = lo << 31 | hi (rows are non-negative int32: 62 bits); bit 62 of the word is the label, 1 = match;
 *   - orientation: under link_only (lo, hi) = (left-table row, right-table row) as given; otherwise both rows index
 *     table 0 and (lo, hi) = (min, max).  The rule holds for a label and for a candidate pair alike, so the order
 *     in which a labelled pair is given does not matter;
 *   - home slot = fmix64(key) & (capacity - 1), fmix64 = MurmurHash3's 64-bit finaliser
 *     (k ^= k >> 33; k *= 0xff51afd7ed558ccd; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53; k ^= k >> 33).
 * out_label_code[i] (optional) is the packed code of the candidate pair that label i names, -1 when blocking did not
 * produce it; if a hand-loaded pair set repeats that pair, the largest of its codes.  out_pattern_mp as for
 * spk_label_histogram (the same device function as spk_score, bit for bit; NULL without m / u).
 * SPK_E_INVALID: NULL rows_l / rows_r / is_match with n_labels > 0; NULL out_counts; out_pattern_mp without m / u; an
 * is_match other than 0 / 1; a row outside its table; l == r on a one-table job; a pair given twice (in either order
 * on a one-table job) -- the last four are found on the device before any pair is counted.  SPK_E_STATE: no
 * comparison codes; no pair rows (a loaded gamma table); a candidate pair that names a row outside its table or a
 * code outside the pattern space (it is not counted).  SPK_E_LIMIT: more than 2^27 labels; 3 * n_patterns > 2^30.
 * Reads the pairs and the codes only: no selection, score, tf, EM or component state is touched, and every device
 * buffer of the call is freed before it returns. */
int spk_label_pairs_histogram(spk_ctx *ctx, int64_t n_labels,
                              const int32_t *rows_l, const int32_t *rows_r /* host, device row order */,
                              const uint8_t *is_match                      /* host, 0 / 1 */,
                              double lambda, double one_minus, const double *m, const double *u,
                              uint64_t *out_counts     /* host [SPK_LABEL_STATES x n_patterns], state-major */,
                              double   *out_pattern_mp /* host [n_patterns] or NULL */,
                              int32_t  *out_label_code /* host [n_labels] or NULL */);
/* The last spk_label_pairs_histogram: pairs counted; with timing on the device milliseconds of its launches (table
 * clear, build, pattern table, counter clear and the histogram; the uploads and read-backs are not in it), -1.0
 * otherwise; the table's capacity in slots; the longest insert probe (slots an insert looked at, its home slot
 * included; 0 without labels).  -1 / -1.0 / -1 / -1: none yet, or the last call failed. */
int spk_label_pairs_info(spk_ctx *ctx, int64_t *out_pairs, double *out_ms, int64_t *out_capacity, int *out_max_probe);

/* ---- scores against labels, per pair (replaces taking the frame make_adjustment_for_term_frequencies returns, or a
 *      filtered frame, to the host with the label column retained and counting the confusion matrix there) ---- */
#define SPK_LABEL_SCORE_MAX_THRESHOLDS 1024
/* Pairs per (truth state, score bin) where the score is decided per pair.  thresholds[0 .. n_thresholds) are ascending
 * doubles (duplicates and +-inf allowed, n_thresholds 0..SPK_LABEL_SCORE_MAX_THRESHOLDS); bin(s) = the number of k with
 * s > thresholds[k], the strict test of SPK_SEL_GT on the same doubles, so it lies in 0..n_thresholds; a NaN (NULL)
 * score falls in bin n_thresholds + 1.  out_counts[s * (n_thresholds + 2) + bin], state-major, states and label ids
 * as for spk_label_histogram (one id per record in device row order, negative = NULL, narrowed to 32 bits on the
 * device: an id >= 2^31 is SPK_E_INVALID; label_ids1 may be NULL unless the job is link_only).  The counts are exact
 * integers that do not depend on launch shape or on the arrival order of the atomics: ranks holding shards sum them.
 *
 * spk_label_scores_tf* (replaces spk_tf_apply* over every pair followed by a host group-by with the labels): every
 * pair of the context, scored by tf_adjusted_match_prob under lambda / one_minus / m / u and the given value ids and
 * tables -- host value ids as for spk_tf_apply, device dictionary ids of the columns `cols` as for
 * spk_tf_apply_columns.  The value is the one spk_tf_apply* gives for the pair, bit for bit (one shared device
 * function); mp comes from a pattern table built for the call, never from spk_score's scores.  m and u are required,
 * n_tf_cols is 1..8, and the context needs codes and a pair set with rows (SPK_E_STATE for a loaded gamma table).
 * Nothing of P elements is stored.
 * SPK_E_INVALID: NULL label_ids0; NULL label_ids1 under link_only; NULL out_counts; more than
 * SPK_LABEL_SCORE_MAX_THRESHOLDS thresholds, a NaN threshold or a descending pair of them; an id >= 2^31.
 * SPK_E_STATE also when a pair names a row outside its table or a code outside the pattern space (it is not counted).
 * The calls read the pairs, codes and tables (spk_label_scores_selection: the selection) and write nothing of the
 * context but the numbers of spk_label_scores_info: the selection, the scores of spk_score, the device-resident tf
 * results, the tf sums, EM and component state are untouched, and every device buffer of a call is freed before it
 * returns. */
int spk_label_scores_tf(spk_ctx *ctx, const int64_t *label_ids0, const int64_t *label_ids1, double lambda,
                        double one_minus, const double *m, const double *u, int n_tf_cols,
                        const int64_t *const *ids_side0, const int64_t *const *ids_side1,
                        const double *const *adj_tables, const int64_t *table_sizes, int n_thresholds,
                        const double *thresholds,
                        uint64_t *out_counts /* host [SPK_LABEL_STATES x (n_thresholds + 2)], state-major */);
int spk_label_scores_tf_columns(spk_ctx *ctx, const int64_t *label_ids0, const int64_t *label_ids1, double lambda,
                                double one_minus, const double *m, const double *u, int n_tf_cols, const int32_t *cols,
                                const double *const *adj_tables, const int64_t *table_sizes, int n_thresholds,
                                const double *thresholds, uint64_t *out_counts);
/* The same over the survivors of the context's selection, one narrowed by spk_select_best included (replaces
 * spk_select_copy* of every survivor followed by the host group-by).  field SPK_SEL_MP: the score is the selection's
 * own match_probability of the survivor's pattern; SPK_SEL_TF_MP: its tf_adjusted_match_prob.  An empty selection is
 * legal and counts nothing.  SPK_E_INVALID: unknown field, and the argument errors above.  SPK_E_STATE: no selection;
 * a stale one; one without pair rows (a loaded gamma table); SPK_SEL_MP on a selection made without m / u;
 * SPK_SEL_TF_MP on one not made by spk_select_tf*. */
int spk_label_scores_selection(spk_ctx *ctx, const int64_t *label_ids0, const int64_t *label_ids1,
                               int field /* SPK_SEL_MP | SPK_SEL_TF_MP */, int n_thresholds, const double *thresholds,
                               uint64_t *out_counts);
/* The last spk_label_scores_*: pairs counted (-1: none yet, or the last call failed), and with timing on
 * (spk_ctx_enable_timing) the device milliseconds of its launches (id narrowing, pattern table, counter clear and
 * the counting kernel; the uploads, the value-id staging and the read-backs are not in it), -1 otherwise. */
int spk_label_scores_info(spk_ctx *ctx, int64_t *out_pairs, double *out_ms);

/* ---- scores against a table of labelled pairs, per pair (replaces taking every tf-scored pair, or every survivor of
 *      a filter or a best-match step, to the host and merging it there with a table of reviewed pairs) ---- */
/* spk_label_scores_*'s counts with the truth state of a pair looked up in a set of n_labels labelled pairs, as
 * spk_label_pairs_histogram looks it up: the same table, key, orientation rule, hash and capacity rule; MATCH and
 * NON_MATCH hold the labelled pairs, UNKNOWN every pair without a label; n_labels = 0 is legal and makes every pair
 * UNKNOWN.  rows_l / rows_r / is_match as for spk_label_pairs_histogram.  The score of a pair and its bin are those of
 * spk_label_scores_tf* (spk_label_pairs_scores_tf*: every pair of the context, tf_adjusted_match_prob by the one
 * shared device function, bit for bit what spk_tf_apply* gives, mp from a pattern table built for the call and never
 * from spk_score's scores) and of spk_label_scores_selection (spk_label_pairs_scores_selection: the survivors of the
 * selection, `field` SPK_SEL_MP or SPK_SEL_TF_MP): bin(s) = the number of k with s > thresholds[k], a NaN (NULL) score
 * in bin n_thresholds + 1; out_counts[s * (n_thresholds + 2) + bin], state-major.  The three rows sum, bin for bin, to
 * what spk_label_scores_* counts for the same pairs with every label id non-NULL.  The counts are exact integers that
 * do not depend on launch shape or on the arrival order of the atomics: ranks holding shards sum them.
 * out_label_pair[i] (optional) is the index of the pair that label i names -- the context's pair index for
 * spk_label_pairs_scores_tf*, the survivor index (spk_select_copy's) for spk_label_pairs_scores_selection -- and -1
 * when no such pair is among them; if a hand-loaded pair set repeats the pair, the largest index.
 * out_label_score[i] (optional) is the score of exactly that pair, NaN when there is none or its score is NULL.
 * SPK_E_INVALID: NULL rows_l / rows_r / is_match with n_labels > 0; NULL out_counts; more than
 * SPK_LABEL_SCORE_MAX_THRESHOLDS thresholds, a NaN threshold or a descending pair of them; NULL m / u, n_tf_cols outside
 * 1..8 (the tf calls); an unknown field (the selection call); an is_match other than 0 / 1; a row outside its table;
 * l == r on a one-table job; a pair given twice (in either order on a one-table job) -- the last four are found on
 * the device before any pair is counted.  SPK_E_STATE: no comparison codes; no pair rows (a loaded gamma table); a
 * pair that names a row outside its table or a code outside the pattern space (it is not counted); a damaged table;
 * the selection call: no selection, a stale one, SPK_SEL_MP on a selection made without m / u, SPK_SEL_TF_MP on one not
 * made by spk_select_tf*.  SPK_E_LIMIT: more than 2^27 labels.
 * The calls read the pairs, codes and tables (the selection call: the selection) and write nothing of the context but
 * the numbers of spk_label_pairs_scores_info: the selection, the scores of spk_score, the device-resident tf results,
 * the tf sums, EM and component state are untouched, and every device buffer of a call is freed before it returns. */
int spk_label_pairs_scores_tf(spk_ctx *ctx, int64_t n_labels,
                              const int32_t *rows_l, const int32_t *rows_r /* host, device row order */,
                              const uint8_t *is_match                      /* host, 0 / 1 */,
                              double lambda, double one_minus, const double *m, const double *u, int n_tf_cols,
                              const int64_t *const *ids_side0, const int64_t *const *ids_side1,
                              const double *const *adj_tables, const int64_t *table_sizes, int n_thresholds,
                              const double *thresholds,
                              uint64_t *out_counts      /* host [SPK_LABEL_STATES x (n_thresholds + 2)], state-major */,
                              int64_t  *out_label_pair  /* host [n_labels] or NULL */,
                              double   *out_label_score /* host [n_labels] or NULL */);
int spk_label_pairs_scores_tf_columns(spk_ctx *ctx, int64_t n_labels, const int32_t *rows_l, const int32_t *rows_r,
                                      const uint8_t *is_match, double lambda, double one_minus, const double *m,
                                      const double *u, int n_tf_cols, const int32_t *cols,
                                      const double *const *adj_tables, const int64_t *table_sizes, int n_thresholds,
                                      const double *thresholds, uint64_t *out_counts, int64_t *out_label_pair,
                                      double *out_label_score);
int spk_label_pairs_scores_selection(spk_ctx *ctx, int64_t n_labels, const int32_t *rows_l, const int32_t *rows_r,
                                     const uint8_t *is_match, int field /* SPK_SEL_MP | SPK_SEL_TF_MP */,
                                     int n_thresholds, const double *thresholds, uint64_t *out_counts,
                                     int64_t *out_label_pair, double *out_label_score);
/* The last spk_label_pairs_scores_*: pairs counted; with timing on the device milliseconds of its launches (table
 * clear, build, pattern table, counter clear, the counting kernel and the per-label kernel; the uploads, the value-id
 * staging and the read-backs are not in it), -1.0 otherwise; the table's capacity in slots; the longest insert probe
 * (0 without labels).  -1 / -1.0 / -1 / -1: none yet, or the last call failed. */
int spk_label_pairs_scores_info(spk_ctx *ctx, int64_t *out_pairs, double *out_ms, int64_t *out_capacity,
                                int *out_max_probe);

/* ---- term-frequency adjustment (term_frequencies.py:122-168) ------------------- */
/* For value ids of one column (per row, -1 NULL; both sides in one id space) accumulate, over
 * pairs with equal non-null values, Σ mp and count(mp) per value id (n_values slots), after spk_score.
 * The sums are exact and order-free, so they are identical for any run, grid and sharding.  Each value
 * has a scale E_v (spk_tf_scales: ilogb of its largest term + 1, INT32_MIN for none) and is summed in
 * fixed point relative to 2^E_v (20-bit limbs down to 2^(E_v - 260)), so tiny match probabilities keep
 * their relative precision.  Ranks holding shards of the pairs all-reduce the scales with MAX, pass
 * them to the _exact forms, all-reduce the returned accumulators (int64 [n_values x SPK_TF_LIMBS],
 * sum) and convert them with spk_tf_limbs_to_sum; the double forms do all of that for one context. */
#define SPK_TF_LIMBS 14
int spk_tf_accumulate(spk_ctx *ctx, int64_t n_values, const int64_t *ids_side0, const int64_t *ids_side1,
                      double *out_sum, int64_t *out_count);
int spk_tf_scales(spk_ctx *ctx, int64_t n_values, const int64_t *ids_side0, const int64_t *ids_side1,
                  int32_t *out_scale);
int spk_tf_accumulate_exact(spk_ctx *ctx, int64_t n_values, const int64_t *ids_side0, const int64_t *ids_side1,
                            const int32_t *scale, int64_t *out_limbs, int64_t *out_count);
/* Host only (no device): Σ mp per value from (all-reduced) accumulators and their scales. */
int spk_tf_limbs_to_sum(int64_t n_values, const int64_t *limbs, const int32_t *scale, double *out_sum);
/* The same with the value ids taken on the device from a string column's dictionary ids (columns
 * added with spk_table_add_raw_utf8: dense in [0, n_values), one id space for both sides, NULL
 * rows excluded), so no host-side factorisation of the tf column is needed.  spk_tf_column_values
 * gives n_values (SPK_E_STATE for a column without device ids). */
int spk_tf_column_values(spk_ctx *ctx, int col, int64_t *out_n_values);
int spk_tf_accumulate_column(spk_ctx *ctx, int col, int64_t n_values, double *out_sum, int64_t *out_count);
int spk_tf_scales_column(spk_ctx *ctx, int col, int64_t n_values, int32_t *out_scale);
int spk_tf_accumulate_column_exact(spk_ctx *ctx, int col, int64_t n_values, const int32_t *scale,
                                   int64_t *out_limbs, int64_t *out_count);
int spk_tf_apply_columns(spk_ctx *ctx, int n_tf_cols, const int32_t *cols, const double *const *adj_tables,
                         const int64_t *table_sizes, int64_t start, int64_t count, double *out_tf_mp,
                         double *out_adj /* [count x n_tf_cols] or NULL */);
/* tf_adjusted_match_prob = bayes(mp, adj_1, ..., adj_n) (:98-117) with adj_c = table_c[id] for pairs
 * with equal non-null values and 0.5 otherwise.  out (host) [start, start+count); out_tf_mp = NULL keeps
 * the results on the device (as spk_score with out = NULL), read back by range with spk_tf_copy. */
int spk_tf_apply(spk_ctx *ctx, int n_tf_cols, const int64_t *const *ids_side0, const int64_t *const *ids_side1,
                 const double *const *adj_tables, const int64_t *table_sizes, int64_t start, int64_t count,
                 double *out_tf_mp, double *out_adj /* [count x n_tf_cols] or NULL */);
/* Pairs [start, start + count) of the tf_adjusted_match_prob the last spk_tf_apply* call with out_tf_mp = NULL
 * kept on the device (SPK_E_STATE when there is none for the current pair set; the range must lie inside the
 * applied one).  Replaces collecting the reference's tf_adjusted_match_prob column (term_frequencies.py:159-168). */
int spk_tf_copy(spk_ctx *ctx, int64_t start, int64_t count, double *out_tf_mp);
/* How the per-value sums find the (value, pattern) counts: 0 (default) a direct histogram when n_values x
 * n_patterns <= min(2^30, max(4 x pairs, 2^24)), else keys (value x n_patterns + pattern, 32-bit when they fit) + radix sort + run-length
 * encode; 1 always the sort; 2 the sort with 64-bit keys (tests hold the three identical).  No reference
 * counterpart (an implementation choice below term_frequencies.py:49-65). */
int spk_tf_set_mode(spk_ctx *ctx, int mode);

#ifdef __cplusplus
}
#endif
#endif /* SPLINK_HIP_H */
