"""ctypes binding to libsplink_hip.so (the C ABI declared in include/splink_hip.h).

There is no CPU fallback: if the library or a gfx950 device is missing, every product
entry point raises `NativeUnavailable`.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SPLINK_AMD_LIB", os.path.join(_HERE, "libsplink_hip.so"))

SPK_OK = 0
SPK_E_INVALID = -1
SPK_E_HIP = -2
SPK_E_OOM = -3
SPK_E_STATE = -4
SPK_E_LIMIT = -5

LINK_TYPES = {"dedupe_only": 0, "link_only": 1, "link_and_dedupe": 2}

# ---- C structs mirrored as numpy structured dtypes (same layout as splink_hip.h) ----------
OPERAND_DTYPE = np.dtype([("kind", "<i4"), ("side", "<i4"), ("col", "<i4"), ("lit", "<i4"), ("num", "<f8"),
                          ("has_num_default", "<i4"), ("substr_start", "<i4"), ("substr_len", "<i4"),
                          ("pad", "<i4")], align=True)
INSTR_DTYPE = np.dtype([("op", "<i4"), ("a", "<i4"), ("b", "<i4"), ("cmp", "<i4"), ("i0", "<i4"), ("pad", "<i4"),
                        ("t", "<f8")], align=True)
PROGRAM_DTYPE = np.dtype([("n_levels", "<i4"), ("else_level", "<i4"), ("n_when", "<i4"), ("first_when", "<i4")],
                         align=True)
KEY_TERM_DTYPE = np.dtype([("raw_l", "<i4"), ("raw_r", "<i4"), ("l_substr_start", "<i4"), ("l_substr_len", "<i4"),
                           ("r_substr_start", "<i4"), ("r_substr_len", "<i4")], align=True)
assert KEY_TERM_DTYPE.itemsize == 24
# spk_select_term: one comparison of a selection (spk_select)
SELECT_TERM_DTYPE = np.dtype([("field", "<i4"), ("col", "<i4"), ("op", "<i4"), ("pad", "<i4"), ("value", "<f8")],
                             align=True)
assert SELECT_TERM_DTYPE.itemsize == 24
SEL_MP, SEL_GAMMA = 0, 1  # SPK_SEL_MP, SPK_SEL_GAMMA
SEL_TF_MP = 2  # SPK_SEL_TF_MP: tf_adjusted_match_prob (select_tf / select_tf_columns only)
SEL_ALL = -1  # SPK_SEL_ALL: every survivor, whatever its score (components_sweep only)
SWEEP_MAX_LEVELS = 32  # SPK_SWEEP_MAX_LEVELS
SEL_OP = {"<": 0, "<=": 1, ">": 2, ">=": 3, "=": 4, "!=": 5, "is null": 6, "is not null": 7}  # SPK_SEL_LT ..
SELECT_MAX_TERMS = 8  # SPK_SELECT_MAX_TERMS
BEST_L, BEST_R, BEST_EITHER, BEST_MUTUAL = 0, 1, 2, 3  # SPK_BEST_L .. SPK_BEST_MUTUAL (select_best's modes)
SAMPLE_MAX_STRATA = 64  # SPK_SAMPLE_MAX_STRATA
TOP_FIRST, TOP_ASC, TOP_DESC = 0, 1, 2  # SPK_TOP_FIRST, SPK_TOP_ASC, SPK_TOP_DESC (select_top's orders)
# Pair ordinals per count of the selection's compaction.  Mirrored from SEL_CHUNK in csrc/spk_select.hip (the
# library exports no call for it); only the tests' edge sizes depend on it.
SELECT_CHUNK = 2048
# Edges per workgroup step of the components' hooking kernel.  Mirrored from CC_CHUNK in csrc/spk_components.hip
# (256 threads x one 16-byte vector of ids each); only the tests' edge sizes depend on it.
COMPONENTS_CHUNK = 1024
# The forest rounds spk_cluster_bridges runs at most (a spanning tree of depth BRIDGES_MAX_ROUNDS - 1).  Mirrored from
# BR_MAX_ROUNDS in csrc/spk_bridges.hip; only the tests' limit case depends on it.
BRIDGES_MAX_ROUNDS = 4096
COMPONENTS_MAX_PEERS = 64  # SPK_COMPONENTS_MAX_PEERS: label arrays per components_merge call
assert OPERAND_DTYPE.itemsize == 40 and INSTR_DTYPE.itemsize == 32 and PROGRAM_DTYPE.itemsize == 16

OP = {"ISNULL": 1, "NOTNULL": 2, "STR_CMP": 3, "NUM_CMP": 4, "JW": 5, "LEV": 6, "LEVRATIO": 7, "ABSDIFF": 8,
      "PERCDIFF": 9, "CONST": 10, "LEN": 11, "JACCARD": 12, "COSINE": 13, "AND": 20, "OR": 21, "NOT": 22}
CMP = {"=": 0, "==": 0, "!=": 1, "<>": 1, "<": 2, "<=": 3, ">": 4, ">=": 5}

EXPORTS = [
    "spk_last_error", "spk_version", "spk_device_count", "spk_ctx_create", "spk_ctx_destroy", "spk_ctx_set_stream",
    "spk_ctx_sync", "spk_ctx_set_link_type", "spk_ctx_kernel_ms", "spk_ctx_enable_timing", "spk_table_create",
    "spk_table_add_utf8", "spk_table_add_float64", "spk_table_set_rank", "spk_table_set_key", "spk_block",
    "spk_pairs_count", "spk_pairs_copy", "spk_pairs_load", "spk_gammas", "spk_gammas_copy", "spk_gammas_load",
    "spk_n_patterns", "spk_gammas_deferred", "spk_em_histogram", "spk_em_finalize", "spk_em_iteration", "spk_score",
    "spk_tf_accumulate", "spk_tf_apply", "spk_jaro_winkler_sim", "spk_levenshtein", "spk_gammas_exact_counts",
    "spk_jaccard_sim", "spk_cosine_distance",
    "spk_gammas_set_simple", "spk_gammas_exact_list", "spk_gammas_simple_count", "spk_em_set_lane_histogram", "spk_table_set_rank_null",
    "spk_gammas_view_regions", "spk_ctx_lds_per_block", "spk_ctx_memory", "spk_raw_utf8", "spk_raw_i64", "spk_key_build", "spk_rank_from_raw", "spk_cluster", "spk_table_add_raw_utf8",
    "spk_gammas_implied_pairs", "spk_tf_column_values", "spk_tf_accumulate_column", "spk_tf_apply_columns", "spk_tf_copy", "spk_tf_set_mode",
    "spk_tf_accumulate_exact", "spk_tf_accumulate_column_exact", "spk_tf_limbs_to_sum", "spk_tf_scales",
    "spk_tf_scales_column", "spk_raw_utf8_arrow", "spk_raw_utf8_arrow_chunks", "spk_table_digest", "spk_raw_release",
    "spk_em_iteration_start", "spk_em_iteration_wait", "spk_ctx_kernel_ms_done", "spk_em_histogram_async",
    "spk_em_finalize_start", "spk_gammas_exact_ms", "spk_gammas_set_window", "spk_gammas_windows", "spk_gammas_set_streams", "spk_gammas_set_graph",
    "spk_gammas_graph_launches",
    "spk_gammas_set_lev_kernel", "spk_gammas_set_lev_bound",
    "spk_block_residual", "spk_block_residual_info",
    "spk_select", "spk_select_copy", "spk_select_info", "spk_select_release",
    "spk_select_tf", "spk_select_tf_columns", "spk_select_copy_tf",
    "spk_select_best", "spk_select_best_info",
    "spk_select_sample", "spk_select_sample_info",
    "spk_select_top", "spk_select_top_of", "spk_select_top_info",
    "spk_components", "spk_components_edges", "spk_components_copy", "spk_components_info", "spk_components_release",
    "spk_components_sweep", "spk_components_sweep_edges", "spk_components_sweep_copy", "spk_components_sweep_info",
    "spk_components_sweep_release", "spk_components_sweep_set_mode",
    "spk_components_merge", "spk_components_sweep_merge", "spk_components_copy_device",
    "spk_components_sweep_copy_device",
    "spk_cluster_metrics", "spk_cluster_metrics_copy", "spk_cluster_metrics_info",
    "spk_cluster_metrics_set_mode",
    "spk_cluster_bridges", "spk_cluster_bridges_copy", "spk_cluster_bridges_cores_copy", "spk_cluster_bridges_info",
    "spk_label_histogram", "spk_label_info",
    "spk_label_pairs_histogram", "spk_label_pairs_info",
    "spk_label_scores_tf", "spk_label_scores_tf_columns", "spk_label_scores_selection", "spk_label_scores_info",
    "spk_label_pairs_scores_tf", "spk_label_pairs_scores_tf_columns", "spk_label_pairs_scores_selection",
    "spk_label_pairs_scores_info",
    "spk_cluster_agreement", "spk_cluster_agreement_info",
    "spk_pairs_sample", "spk_pairs_sample_info",
    "spk_block_profile", "spk_block_profile_info", "spk_block_profile_set_cut",
    "spk_em_lane_copies",
    "spk_ingest_set_hash_bits",
]
# spk_rule_profile / spk_block_entry: the per-rule figures and one of a rule's largest blocks (spk_block_profile)
RULE_PROFILE_DTYPE = np.dtype([("rows_l", "<i8"), ("rows_r", "<i8"), ("blocks", "<i8"), ("candidates", "<i8"),
                               ("largest_candidates", "<i8"), ("enumerated", "<i8")], align=True)
BLOCK_ENTRY_DTYPE = np.dtype([("rows_l", "<i8"), ("rows_r", "<i8"), ("candidates", "<i8"), ("row_l", "<i4"),
                              ("pad", "<i4")], align=True)
assert RULE_PROFILE_DTYPE.itemsize == 48 and BLOCK_ENTRY_DTYPE.itemsize == 32
PROFILE_BINS = 64  # SPK_PROFILE_BINS
LARGEST_BY_CANDIDATES, LARGEST_BY_ROWS_L = 0, 1  # SPK_LARGEST_BY_*
# Draws per workgroup of spk_pairs_sample's kernel (256 threads x 8 consecutive draws).  Mirrored from SM_CHUNK in
# csrc/spk_sample.hip; only the tests' edge sizes depend on it.
SAMPLE_CHUNK = 2048
LABEL_NON_MATCH, LABEL_MATCH, LABEL_UNKNOWN, LABEL_STATES = 0, 1, 2, 3  # SPK_LABEL_*
# LDS bytes up to which spk_label_histogram keeps its 3 x n_patterns 32-bit counters in the workgroup (capped by
# lds_per_block()); past it the counts go to global memory.  Mirrored from LH_LDS_BYTES in csrc/spk_labels.hip;
# only the tests' choice of pattern spaces depends on it.
LABEL_LDS_BYTES = 64 * 1024
LABEL_PAIRS_MAX = 1 << 27  # labelled pairs one spk_label_pairs_histogram takes
LABEL_SCORE_MAX_THRESHOLDS = 1024  # SPK_LABEL_SCORE_MAX_THRESHOLDS
# Pairs one workgroup of spk_label_scores_tf*'s kernel takes per step (256 threads x 8 pairs) and the workgroups per
# compute unit its grid is capped at.  Mirrored from LS_THREADS, LS_PAIRS and LS_WG_PER_CU in csrc/spk_labels.hip; only
# the tests' edge sizes depend on them.
LABEL_SCORE_STEP = 256 * 8
LABEL_SCORE_WG_PER_CU = 3
# The same for spk_label_pairs_scores_tf*'s kernel.  Mirrored from LS_THREADS, LPS_PAIRS and LPS_WAVES_PER_SIMD.
LABEL_PAIR_SCORE_STEP = 256 * 4
LABEL_PAIR_SCORE_WG_PER_CU = 6
AGREE_FIELDS = 10  # SPK_AGREE_FIELDS: the columns of cluster_agreement, in labels.AGREEMENT_FIELDS' order
TF_LIMBS = 14  # SPK_TF_LIMBS


class NativeUnavailable(RuntimeError):
    """libsplink_hip.so or a gfx950 HIP device is unavailable (there is no CPU fallback)."""


_lib = None


def load_library():
    """Load libsplink_hip.so (no device needed)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeUnavailable(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
    lib = ctypes.CDLL(LIB_PATH)
    lib.spk_last_error.restype = ctypes.c_char_p
    lib.spk_ctx_destroy.restype = None
    for name in EXPORTS:
        getattr(lib, name)  # raises AttributeError when a declared symbol is missing
    _lib = lib
    return lib


def tf_limbs_to_sum(limbs, scale) -> np.ndarray:
    """Σmp per value from fixed-point accumulators and the values' scales (host only, no device)."""
    lib = load_library()
    limbs = np.ascontiguousarray(limbs, dtype=np.int64).reshape(-1, TF_LIMBS)
    scale = np.ascontiguousarray(scale, dtype=np.int32)
    assert len(scale) == len(limbs)
    out = np.zeros(max(len(limbs), 1), dtype=np.float64)
    check(lib.spk_tf_limbs_to_sum(ctypes.c_int64(len(limbs)), _ptr(limbs), _ptr(scale), _ptr(out)),
          "spk_tf_limbs_to_sum")
    return out[:len(limbs)]


TF_NO_SCALE = np.iinfo(np.int32).min  # a value without a positive term


def device_count() -> int:
    lib = load_library()
    n = ctypes.c_int(0)
    lib.spk_device_count(ctypes.byref(n))
    return n.value


def _ptr(a):
    return ctypes.c_void_p(0) if a is None else ctypes.c_void_p(a.ctypes.data)


def check(rc: int, what: str):
    if rc == SPK_OK:
        return
    msg = load_library().spk_last_error().decode("utf-8", "replace")
    if rc in (SPK_E_INVALID, SPK_E_LIMIT):
        raise ValueError(f"{what}: {msg}")
    raise RuntimeError(f"{what} failed ({rc}): {msg}")


class Context:
    """One spk_ctx: one device, one stream, one set of tables / pairs / codes."""

    def __init__(self, device: int = 0):
        lib = load_library()
        if device_count() <= device:
            raise NativeUnavailable(f"no HIP device {device} visible (splink_amd needs an MI355X / gfx950)")
        h = ctypes.c_void_p()
        check(lib.spk_ctx_create(ctypes.c_int(device), ctypes.byref(h)), "spk_ctx_create")
        self._h = h
        self._lib = lib
        self.device = device

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.spk_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- calls ------------------------------------------------------------------------
    def set_stream(self, stream_ptr: int):
        check(self._lib.spk_ctx_set_stream(self._h, ctypes.c_void_p(stream_ptr)), "spk_ctx_set_stream")

    def sync(self):
        check(self._lib.spk_ctx_sync(self._h), "spk_ctx_sync")

    def set_link_type(self, link_type: int):
        check(self._lib.spk_ctx_set_link_type(self._h, ctypes.c_int(link_type)), "spk_ctx_set_link_type")

    def enable_timing(self, on: bool = True, exact: bool = False):
        """HIP-event timing of the kernel families; exact=True also times each column's exact-pass launch."""
        check(self._lib.spk_ctx_enable_timing(self._h, ctypes.c_int((2 if exact else 1) if on else 0)),
              "spk_ctx_enable_timing")

    def kernel_ms(self):
        out = np.zeros(5, dtype=np.float64)
        check(self._lib.spk_ctx_kernel_ms(self._h, _ptr(out)), "spk_ctx_kernel_ms")
        return dict(zip(["block", "gamma", "em_hist", "em_final", "score"], out.tolist()))

    def kernel_ms_done(self):
        """kernel_ms without synchronising: per family the newest launch that has completed (-1 = none)."""
        out = np.zeros(5, dtype=np.float64)
        check(self._lib.spk_ctx_kernel_ms_done(self._h, _ptr(out)), "spk_ctx_kernel_ms_done")
        return dict(zip(["block", "gamma", "em_hist", "em_final", "score"], out.tolist()))

    def table_create(self, side: int, n_rows: int, n_cols: int):
        check(self._lib.spk_table_create(self._h, ctypes.c_int(side), ctypes.c_int64(n_rows), ctypes.c_int(n_cols)),
              "spk_table_create")

    def table_add_utf8(self, side, col, offsets, data, valid, value_ids=None):
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        data = np.ascontiguousarray(data, dtype=np.uint8)
        if data.size == 0:
            data = np.zeros(1, dtype=np.uint8)
        valid = np.ascontiguousarray(valid, dtype=np.uint8)
        ids = None if value_ids is None else np.ascontiguousarray(value_ids, dtype=np.int64)
        check(self._lib.spk_table_add_utf8(self._h, ctypes.c_int(side), ctypes.c_int(col), _ptr(offsets), _ptr(data),
                                           _ptr(valid), _ptr(ids)), "spk_table_add_utf8")

    def table_add_float64(self, side, col, values, valid):
        values = np.ascontiguousarray(values, dtype=np.float64)
        valid = np.ascontiguousarray(valid, dtype=np.uint8)
        check(self._lib.spk_table_add_float64(self._h, ctypes.c_int(side), ctypes.c_int(col), _ptr(values),
                                              _ptr(valid)), "spk_table_add_float64")

    def table_set_rank(self, side, rank):
        rank = np.ascontiguousarray(rank, dtype=np.int64)
        check(self._lib.spk_table_set_rank(self._h, ctypes.c_int(side), _ptr(rank)), "spk_table_set_rank")

    def table_set_rank_null(self, side, divisor):
        check(self._lib.spk_table_set_rank_null(self._h, ctypes.c_int(side), ctypes.c_int64(divisor)),
              "spk_table_set_rank_null")

    # ---- device ingest ---------------------------------------------------------------------
    def raw_utf8(self, raw, offsets, data, valid):
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        data = np.ascontiguousarray(data, dtype=np.uint8)
        if data.size == 0:
            data = np.zeros(1, dtype=np.uint8)
        valid = np.ascontiguousarray(valid, dtype=np.uint8)
        check(self._lib.spk_raw_utf8(self._h, ctypes.c_int(raw), ctypes.c_int64(len(offsets) - 1), _ptr(offsets),
                                     _ptr(data), _ptr(valid)), "spk_raw_utf8")

    def raw_utf8_arrow(self, raw, n, offsets, data, bitmap=None, bit_offset=0):
        """Arrow buffers as numpy views (no copies): offsets int64[n+1] (any base), data uint8, validity bitmap
        (None = no NULLs; bit_offset -1 = one byte per row)."""
        check(self._lib.spk_raw_utf8_arrow(self._h, ctypes.c_int(raw), ctypes.c_int64(n), _ptr(offsets), _ptr(data),
                                           _ptr(bitmap), ctypes.c_int64(bit_offset), ctypes.c_int(0)),
              "spk_raw_utf8_arrow")

    def raw_utf8_arrow_chunks(self, raw, views, rows):
        """A chunked Arrow column: views[c] = arrow_views(chunk c) (offsets, data, bitmap or None, bit offset),
        rows[c] its row count; the chunks' rows are concatenated on the device."""
        nc = len(views)
        c_rows = (ctypes.c_int64 * nc)(*[int(r) for r in rows])
        c_off = (ctypes.c_void_p * nc)(*[_ptr(v[0]).value for v in views])
        c_data = (ctypes.c_void_p * nc)(*[_ptr(v[1]).value for v in views])
        c_valid = (ctypes.c_void_p * nc)(*[_ptr(v[2]).value if v[2] is not None else None for v in views])
        c_bit = (ctypes.c_int64 * nc)(*[int(v[3]) if v[2] is not None else 0 for v in views])
        check(self._lib.spk_raw_utf8_arrow_chunks(self._h, ctypes.c_int(raw), ctypes.c_int(nc), c_rows, c_off, c_data,
                                                  c_valid, c_bit), "spk_raw_utf8_arrow_chunks")

    def raw_utf8_device(self, raw, n, d_offsets, d_data, d_valid_bytes):
        """The same from device buffers (int pointers: offsets int64[n+1], data, one validity byte per row)."""
        check(self._lib.spk_raw_utf8_arrow(self._h, ctypes.c_int(raw), ctypes.c_int64(n), ctypes.c_void_p(d_offsets),
                                           ctypes.c_void_p(d_data), ctypes.c_void_p(d_valid_bytes),
                                           ctypes.c_int64(-1), ctypes.c_int(1)), "spk_raw_utf8_arrow")

    def raw_release(self, raw: int):
        check(self._lib.spk_raw_release(self._h, ctypes.c_int(raw)), "spk_raw_release")

    def table_digest(self, side: int) -> int:
        out = ctypes.c_uint64(0)
        check(self._lib.spk_table_digest(self._h, ctypes.c_int(side), ctypes.byref(out)), "spk_table_digest")
        return out.value

    def raw_i64(self, raw, values, valid):
        values = np.ascontiguousarray(values, dtype=np.int64)
        valid = np.ascontiguousarray(valid, dtype=np.uint8)
        if values.size == 0:
            values, valid = np.zeros(1, np.int64), np.zeros(1, np.uint8)
            n = 0
        else:
            n = len(values)
        check(self._lib.spk_raw_i64(self._h, ctypes.c_int(raw), ctypes.c_int64(n), _ptr(values), _ptr(valid)),
              "spk_raw_i64")

    def key_build(self, rule, terms):
        t = np.array([tuple(x) for x in terms], dtype=KEY_TERM_DTYPE)
        check(self._lib.spk_key_build(self._h, ctypes.c_int(rule), ctypes.c_int(len(t)), _ptr(t)), "spk_key_build")

    def ingest_set_hash_bits(self, bits: int):
        """Width (1 .. 63 bits, default 63) of the hash behind key_build's and table_add_raw_utf8's dense ids:
        tests reach the collision check, the retry under the next seed and the error after four with it."""
        check(self._lib.spk_ingest_set_hash_bits(self._h, ctypes.c_int(int(bits))), "spk_ingest_set_hash_bits")

    def rank_from_raw(self, raw_uid, right_from=-1):
        check(self._lib.spk_rank_from_raw(self._h, ctypes.c_int(raw_uid), ctypes.c_int64(right_from)),
              "spk_rank_from_raw")

    def cluster(self, n0, n1=None):
        p0 = np.empty(max(n0, 1), dtype=np.int32)
        p1 = np.empty(max(n1 or 0, 1), dtype=np.int32) if n1 is not None else None
        check(self._lib.spk_cluster(self._h, _ptr(p0), _ptr(p1)), "spk_cluster")
        return p0[:n0], (p1[:n1] if p1 is not None else None)

    def table_add_raw_utf8(self, col, raw0, raw1=-1):
        check(self._lib.spk_table_add_raw_utf8(self._h, ctypes.c_int(col), ctypes.c_int(raw0), ctypes.c_int(raw1)),
              "spk_table_add_raw_utf8")

    def table_set_key(self, side, rule, which, keys):
        keys = np.ascontiguousarray(keys, dtype=np.int64)
        check(self._lib.spk_table_set_key(self._h, ctypes.c_int(side), ctypes.c_int(rule), ctypes.c_int(which),
                                          _ptr(keys)), "spk_table_set_key")

    def block(self, link_type: int, symmetric, shard: int = 0, n_shards: int = 1):
        sym = np.ascontiguousarray(symmetric, dtype=np.int32)
        n_pairs = ctypes.c_int64(0)
        n_total = ctypes.c_int64(0)
        check(self._lib.spk_block(self._h, ctypes.c_int(link_type), ctypes.c_int(len(sym)), _ptr(sym),
                                  ctypes.c_int(shard), ctypes.c_int(n_shards), ctypes.byref(n_pairs),
                                  ctypes.byref(n_total)), "spk_block")
        return n_pairs.value, n_total.value

    def block_residual(self, link_type: int, symmetric, rule_program, args, shard: int = 0, n_shards: int = 1):
        """spk_block_residual: rules with residual predicates.  rule_program[r]: index of rule r's hidden program
        in `args` (gammas_args of the rules' predicates), -1 for a rule that is only its key equalities."""
        sym = np.ascontiguousarray(symmetric, dtype=np.int32)
        prog = np.ascontiguousarray(rule_program, dtype=np.int32)
        assert len(prog) == len(sym)
        n_pairs = ctypes.c_int64(0)
        n_total = ctypes.c_int64(0)
        check(self._lib.spk_block_residual(self._h, ctypes.c_int(link_type), ctypes.c_int(len(sym)), _ptr(sym),
                                           _ptr(prog), ctypes.c_int(shard), ctypes.c_int(n_shards), *args[1],
                                           ctypes.byref(n_pairs), ctypes.byref(n_total)), "spk_block_residual")
        return n_pairs.value, n_total.value

    def block_residual_info(self):
        """(pairs the last block_residual enumerated before its filter, ms of its compaction kernels or -1)."""
        n = ctypes.c_int64(0)
        ms = ctypes.c_double(-1.0)
        check(self._lib.spk_block_residual_info(self._h, ctypes.byref(n), ctypes.byref(ms)), "spk_block_residual_info")
        return n.value, ms.value

    def block_profile(self, link_type: int, symmetric, rule_program=None, shard: int = 0, n_shards: int = 1,
                      max_enumerate: int = 0, largest_by: int = LARGEST_BY_CANDIDATES, limit: int = 5):
        """spk_block_profile over the rules whose keys are set: (rules [n_rules] of RULE_PROFILE_DTYPE, histogram
        int64 [n_rules, PROFILE_BINS, 2] of (blocks, candidates) per bit length of a block's candidate count, and per
        rule its largest blocks as an array of BLOCK_ENTRY_DTYPE).  The pair set and the rest of the context stay."""
        sym = np.ascontiguousarray(symmetric, dtype=np.int32)
        prog = None if rule_program is None else np.ascontiguousarray(rule_program, dtype=np.int32)
        assert prog is None or len(prog) == len(sym)
        n, limit = len(sym), int(limit)
        rules = np.zeros(max(n, 1), dtype=RULE_PROFILE_DTYPE)
        hist = np.zeros((max(n, 1), PROFILE_BINS, 2), dtype=np.int64)
        largest = np.zeros((max(n, 1), max(limit, 1)), dtype=BLOCK_ENTRY_DTYPE)
        n_largest = np.zeros(max(n, 1), dtype=np.int32)
        check(self._lib.spk_block_profile(self._h, ctypes.c_int(link_type), ctypes.c_int(n), _ptr(sym), _ptr(prog),
                                          ctypes.c_int(shard), ctypes.c_int(n_shards),
                                          ctypes.c_int64(int(max_enumerate)), ctypes.c_int(int(largest_by)),
                                          ctypes.c_int(limit), _ptr(rules), _ptr(hist), _ptr(largest),
                                          _ptr(n_largest)), "spk_block_profile")
        return rules[:n], hist[:n], [largest[r, :int(n_largest[r])].copy() for r in range(n)]

    def block_profile_info(self):
        """(ms of the last block_profile's key-level part, ms of its enumeration -- HIP events, timing on, else -1 --
        and the ordinals its count pass went through, -1: none yet or the last call failed)."""
        key_ms = ctypes.c_double(-1.0)
        enum_ms = ctypes.c_double(-1.0)
        n = ctypes.c_int64(-1)
        check(self._lib.spk_block_profile_info(self._h, ctypes.byref(key_ms), ctypes.byref(enum_ms), ctypes.byref(n)),
              "spk_block_profile_info")
        return key_ms.value, enum_ms.value, n.value

    def block_profile_set_cut(self, on: bool = True):
        """Measurement switch: False sorts every block in the largest-blocks step instead of the top bins' only."""
        check(self._lib.spk_block_profile_set_cut(self._h, ctypes.c_int(1 if on else 0)), "spk_block_profile_set_cut")

    def pairs_count(self) -> int:
        n = ctypes.c_int64(0)
        check(self._lib.spk_pairs_count(self._h, ctypes.byref(n)), "spk_pairs_count")
        return n.value

    def pairs_copy(self, start: int = 0, count: int | None = None):
        if count is None:
            count = self.pairs_count() - start
        l = np.empty(count, dtype=np.int32)
        r = np.empty(count, dtype=np.int32)
        check(self._lib.spk_pairs_copy(self._h, ctypes.c_int64(start), ctypes.c_int64(count), _ptr(l), _ptr(r)),
              "spk_pairs_copy")
        return l, r

    def pairs_load(self, rows_l, rows_r):
        rows_l = np.ascontiguousarray(rows_l, dtype=np.int32)
        rows_r = np.ascontiguousarray(rows_r, dtype=np.int32)
        check(self._lib.spk_pairs_load(self._h, ctypes.c_int64(len(rows_l)), _ptr(rows_l), _ptr(rows_r)),
              "spk_pairs_load")

    def pairs_sample(self, link_type: int, seed: int, total: int, first: int, count: int) -> int:
        """spk_pairs_sample: replace the pair set by the surviving draws among the ordinals [first, first + count)
        of a random sample of `total` draws under `seed` (with replacement; splink_hip.h has the definition);
        returns how many pairs survive."""
        n = ctypes.c_int64(0)
        check(self._lib.spk_pairs_sample(self._h, ctypes.c_int(int(link_type)),
                                         ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), ctypes.c_int64(int(total)),
                                         ctypes.c_int64(int(first)), ctypes.c_int64(int(count)), ctypes.byref(n)),
              "spk_pairs_sample")
        return n.value

    def pairs_sample_info(self):
        """(draws of the last pairs_sample or -1, pairs it kept or -1, ms of its launches with timing on or -1)."""
        d = ctypes.c_int64(-1)
        k = ctypes.c_int64(-1)
        ms = ctypes.c_double(-1.0)
        check(self._lib.spk_pairs_sample_info(self._h, ctypes.byref(d), ctypes.byref(k), ctypes.byref(ms)),
              "spk_pairs_sample_info")
        return d.value, k.value, ms.value

    @staticmethod
    def gammas_args(programs, when_first, when_n, when_level, instrs, operands, lit_offsets, lit_bytes):
        """The spk_gammas argument list, converted once (cached by the caller across calls)."""
        programs = np.ascontiguousarray(programs, dtype=PROGRAM_DTYPE)
        wf = np.ascontiguousarray(when_first, dtype=np.int32)
        wn = np.ascontiguousarray(when_n, dtype=np.int32)
        wl = np.ascontiguousarray(when_level, dtype=np.int32)
        instrs = np.ascontiguousarray(instrs, dtype=INSTR_DTYPE)
        operands = np.ascontiguousarray(operands, dtype=OPERAND_DTYPE)
        lo = np.ascontiguousarray(lit_offsets, dtype=np.int64)
        lb = np.ascontiguousarray(lit_bytes, dtype=np.uint8)
        if lb.size == 0:
            lb = np.zeros(1, dtype=np.uint8)
        keep = (programs, wf, wn, wl, instrs, operands, lo, lb)
        c_args = (ctypes.c_int(len(programs)), _ptr(programs), ctypes.c_int(len(wf)), _ptr(wf), _ptr(wn), _ptr(wl),
                  ctypes.c_int(len(instrs)), _ptr(instrs), ctypes.c_int(len(operands)), _ptr(operands),
                  ctypes.c_int(len(lo) - 1), _ptr(lo), _ptr(lb))
        return keep, c_args

    def gammas_native(self, args):
        check(self._lib.spk_gammas(self._h, *args[1]), "spk_gammas")

    def gammas(self, programs, when_first, when_n, when_level, instrs, operands, lit_offsets, lit_bytes):
        programs = np.ascontiguousarray(programs, dtype=PROGRAM_DTYPE)
        wf = np.ascontiguousarray(when_first, dtype=np.int32)
        wn = np.ascontiguousarray(when_n, dtype=np.int32)
        wl = np.ascontiguousarray(when_level, dtype=np.int32)
        instrs = np.ascontiguousarray(instrs, dtype=INSTR_DTYPE)
        operands = np.ascontiguousarray(operands, dtype=OPERAND_DTYPE)
        lo = np.ascontiguousarray(lit_offsets, dtype=np.int64)
        lb = np.ascontiguousarray(lit_bytes, dtype=np.uint8)
        if lb.size == 0:
            lb = np.zeros(1, dtype=np.uint8)
        check(self._lib.spk_gammas(self._h, ctypes.c_int(len(programs)), _ptr(programs), ctypes.c_int(len(wf)),
                                   _ptr(wf), _ptr(wn), _ptr(wl), ctypes.c_int(len(instrs)), _ptr(instrs),
                                   ctypes.c_int(len(operands)), _ptr(operands), ctypes.c_int(len(lo) - 1), _ptr(lo),
                                   _ptr(lb)), "spk_gammas")

    def gammas_load(self, n_levels, gammas):
        nl = np.ascontiguousarray(n_levels, dtype=np.int32)
        g = np.ascontiguousarray(gammas, dtype=np.int8)
        check(self._lib.spk_gammas_load(self._h, ctypes.c_int(len(nl)), _ptr(nl), ctypes.c_int64(g.shape[0]), _ptr(g)),
              "spk_gammas_load")

    def gammas_copy(self, K: int, start: int, count: int):
        out = np.empty((count, K), dtype=np.int8)
        check(self._lib.spk_gammas_copy(self._h, ctypes.c_int64(start), ctypes.c_int64(count), _ptr(out)),
              "spk_gammas_copy")
        return out

    def n_patterns(self) -> int:
        n = ctypes.c_int64(0)
        check(self._lib.spk_n_patterns(self._h, ctypes.byref(n)), "spk_n_patterns")
        return n.value

    def gammas_deferred(self) -> int:
        n = ctypes.c_int64(0)
        check(self._lib.spk_gammas_deferred(self._h, ctypes.byref(n)), "spk_gammas_deferred")
        return n.value

    def gammas_exact_counts(self, K: int):
        out = np.zeros(max(K, 1), dtype=np.int64)
        check(self._lib.spk_gammas_exact_counts(self._h, _ptr(out), ctypes.c_int(len(out))), "spk_gammas_exact_counts")
        return out[:K].tolist()

    def gammas_exact_list(self, k: int, n: int):
        out = np.empty(int(n), dtype=np.int32)
        check(self._lib.spk_gammas_exact_list(self._h, ctypes.c_int(k), _ptr(out), ctypes.c_int64(int(n))),
              "spk_gammas_exact_list")
        return out

    def gammas_implied_pairs(self, K: int):
        out = np.zeros(max(K, 1), dtype=np.int64)
        check(self._lib.spk_gammas_implied_pairs(self._h, _ptr(out), ctypes.c_int(len(out))), "spk_gammas_implied_pairs")
        return out[:K].tolist()

    def gammas_set_simple(self, mode):
        """1 / True: template-shaped columns through the filter kernel, 0: every column through the interpreter;
        + 10: rule 1's pairs never read the view-ordered image, + 20: always (tests)."""
        check(self._lib.spk_gammas_set_simple(self._h, ctypes.c_int(int(mode))), "spk_gammas_set_simple")

    def gammas_set_window(self, pairs: int):
        """Cap spk_gammas' ordinal windows at `pairs` (0 = default, just under 2^31; for testing)."""
        check(self._lib.spk_gammas_set_window(self._h, ctypes.c_int64(int(pairs))), "spk_gammas_set_window")

    def gammas_set_streams(self, streams: int, min_pairs: int = 1 << 22):
        """spk_gammas' two-stream split: 2 streams (default) for pair sets of at least min_pairs, or 1."""
        check(self._lib.spk_gammas_set_streams(self._h, ctypes.c_int(int(streams)), ctypes.c_int64(int(min_pairs))),
              "spk_gammas_set_streams")

    def gammas_set_graph(self, on: bool):
        """Replay unchanged comparison passes from a captured HIP graph (default off: slower than direct launches)."""
        check(self._lib.spk_gammas_set_graph(self._h, ctypes.c_int(1 if on else 0)), "spk_gammas_set_graph")

    def gammas_graph_launches(self) -> int:
        n = ctypes.c_int64(0)
        check(self._lib.spk_gammas_graph_launches(self._h, ctypes.byref(n)), "spk_gammas_graph_launches")
        return n.value

    def gammas_windows(self) -> int:
        n = ctypes.c_int64(0)
        check(self._lib.spk_gammas_windows(self._h, ctypes.byref(n)), "spk_gammas_windows")
        return n.value

    def gammas_set_lev_kernel(self, mode: int):
        """Levenshtein exact pass (same codes; A/B tests): 2 lane refill in free-text columns, one cell per lane
        elsewhere (default); 1 lane refill everywhere; 0 one cell per lane everywhere; 3 as 2 without the
        character-bag decisions before the refill pass."""
        check(self._lib.spk_gammas_set_lev_kernel(self._h, ctypes.c_int(int(mode))), "spk_gammas_set_lev_kernel")

    def gammas_set_lev_bound(self, mode: int):
        """Filter field of template Levenshtein columns without free-text rows (same codes; A/B tests): 1 the
        positional sketch and its two-segment bound (default), 0 key, lengths and the whole-string sketch."""
        check(self._lib.spk_gammas_set_lev_bound(self._h, ctypes.c_int(int(mode))), "spk_gammas_set_lev_bound")

    def lds_per_block(self) -> int:
        n = ctypes.c_int(0)
        check(self._lib.spk_ctx_lds_per_block(self._h, ctypes.byref(n)), "spk_ctx_lds_per_block")
        return n.value

    MEMORY_PARTS = ("raw_columns", "record_encodings", "row_images", "pairs", "codes", "work_lists", "em_score_tf",
                    "total")

    def memory(self) -> dict:
        """Device bytes the context holds, by what they store (spk_ctx_memory)."""
        out = np.zeros(8, dtype=np.int64)
        check(self._lib.spk_ctx_memory(self._h, _ptr(out)), "spk_ctx_memory")
        return dict(zip(self.MEMORY_PARTS, [int(x) for x in out]))

    def gammas_view_regions(self) -> int:
        n = ctypes.c_int64(0)
        check(self._lib.spk_gammas_view_regions(self._h, ctypes.byref(n)), "spk_gammas_view_regions")
        return n.value

    def gammas_exact_ms(self, n: int):
        out = np.zeros(max(n, 1), dtype=np.float64)
        check(self._lib.spk_gammas_exact_ms(self._h, _ptr(out), ctypes.c_int(n)), "spk_gammas_exact_ms")
        return out[:n].tolist()

    def gammas_simple_count(self) -> int:
        n = ctypes.c_int(0)
        check(self._lib.spk_gammas_simple_count(self._h, ctypes.byref(n)), "spk_gammas_simple_count")
        return n.value

    def em_set_lane_histogram(self, on):
        """True / 1: lane-private counters, release fence before each last-arriver ticket (default); False / 0:
        wave-ballot histogram; 2: lane counters without the fence (A/B)."""
        check(self._lib.spk_em_set_lane_histogram(self._h, ctypes.c_int(int(on))), "spk_em_set_lane_histogram")

    def em_lane_copies(self) -> int:
        """Lane-private copies per pattern of the E+M launch for the current pairs and pattern space (64 .. 4);
        0: the wave-ballot histogram + finalize launches."""
        n = ctypes.c_int(0)
        check(self._lib.spk_em_lane_copies(self._h, ctypes.byref(n)), "spk_em_lane_copies")
        return n.value

    def em_histogram(self, d_hist_ptr: int = 0):
        check(self._lib.spk_em_histogram(self._h, ctypes.c_void_p(d_hist_ptr)), "spk_em_histogram")

    def em_histogram_async(self, d_hist_ptr: int):
        check(self._lib.spk_em_histogram_async(self._h, ctypes.c_void_p(d_hist_ptr)), "spk_em_histogram_async")

    def em_finalize_start(self, d_hist_ptr, lam, one_minus, m, u, n_stats):
        m = np.ascontiguousarray(m, dtype=np.float64)
        u = np.ascontiguousarray(u, dtype=np.float64)
        check(self._lib.spk_em_finalize_start(self._h, ctypes.c_void_p(d_hist_ptr), ctypes.c_double(lam),
                                              ctypes.c_double(one_minus), _ptr(m), _ptr(u), ctypes.c_int(n_stats)),
              "spk_em_finalize_start")

    def em_finalize(self, d_hist_ptr, lam, one_minus, m, u, n_stats):
        m = np.ascontiguousarray(m, dtype=np.float64)
        u = np.ascontiguousarray(u, dtype=np.float64)
        out = np.zeros(n_stats, dtype=np.float64)
        check(self._lib.spk_em_finalize(self._h, ctypes.c_void_p(d_hist_ptr), ctypes.c_double(lam),
                                        ctypes.c_double(one_minus), _ptr(m), _ptr(u), _ptr(out),
                                        ctypes.c_int(n_stats)), "spk_em_finalize")
        return out

    def em_iteration(self, lam, one_minus, m, u, n_stats):
        """One E+M iteration on this GPU's pairs in one launch (histogram, E-step per pattern, M-step sums)."""
        m = np.ascontiguousarray(m, dtype=np.float64)
        u = np.ascontiguousarray(u, dtype=np.float64)
        out = self._stats_buf(n_stats)
        check(self._lib.spk_em_iteration(self._h, ctypes.c_double(lam), ctypes.c_double(one_minus), _ptr(m), _ptr(u),
                                         _ptr(out), ctypes.c_int(n_stats)), "spk_em_iteration")
        return out

    def em_iteration_start(self, lam, one_minus, m, u, n_stats):
        """Enqueue one E+M iteration (spk_em_iteration_start); em_iteration_wait returns its statistics."""
        m = np.ascontiguousarray(m, dtype=np.float64)
        u = np.ascontiguousarray(u, dtype=np.float64)
        check(self._lib.spk_em_iteration_start(self._h, ctypes.c_double(lam), ctypes.c_double(one_minus), _ptr(m),
                                               _ptr(u), ctypes.c_int(n_stats)), "spk_em_iteration_start")

    def em_iteration_wait(self, n_stats):
        out = self._stats_buf(n_stats)
        check(self._lib.spk_em_iteration_wait(self._h, _ptr(out), ctypes.c_int(n_stats)), "spk_em_iteration_wait")
        return out

    def _stats_buf(self, n_stats):
        return np.zeros(n_stats, dtype=np.float64)

    def score(self, lam, one_minus, m, u, start=0, count=0, want_host=True):
        m = np.ascontiguousarray(m, dtype=np.float64)
        u = np.ascontiguousarray(u, dtype=np.float64)
        out = np.empty(count, dtype=np.float64) if want_host else None
        check(self._lib.spk_score(self._h, ctypes.c_double(lam), ctypes.c_double(one_minus), _ptr(m), _ptr(u),
                                  ctypes.c_int64(start), ctypes.c_int64(count), _ptr(out)), "spk_score")
        return out

    # ---- selection of scored pairs ------------------------------------------------------------
    def select(self, lam, one_minus, m, u, terms) -> int:
        """spk_select: keep the pairs for which every term (field, col, op, value) is TRUE; returns how many.
        m = u = None when no term reads match_probability (the survivors then carry none)."""
        t = np.zeros(len(terms), dtype=SELECT_TERM_DTYPE)
        for i, (field, col, op, value) in enumerate(terms):
            t[i] = (field, col, op, 0, value)
        m = None if m is None else np.ascontiguousarray(m, dtype=np.float64)
        u = None if u is None else np.ascontiguousarray(u, dtype=np.float64)
        n = ctypes.c_int64(0)
        check(self._lib.spk_select(self._h, ctypes.c_double(lam), ctypes.c_double(one_minus), _ptr(m), _ptr(u),
                                   ctypes.c_int(len(t)), _ptr(t) if len(t) else ctypes.c_void_p(0), ctypes.byref(n)),
              "spk_select")
        return n.value

    @staticmethod
    def _select_terms(terms):
        t = np.zeros(len(terms), dtype=SELECT_TERM_DTYPE)
        for i, (field, col, op, value) in enumerate(terms):
            t[i] = (field, col, op, 0, value)
        return t

    def select_tf(self, lam, one_minus, m, u, ids0_list, ids1_list, tables, terms) -> int:
        """spk_select_tf: select as `select`, with terms on tf_adjusted_match_prob (field SEL_TF_MP) under the given
        host value ids per row and adjustment tables (as tf_apply); returns how many pairs are kept."""
        n = len(tables)
        keep = [np.ascontiguousarray(a, dtype=np.int64) for a in ids0_list] + \
               [np.ascontiguousarray(a, dtype=np.int64) for a in ids1_list] + \
               [np.ascontiguousarray(t, dtype=np.float64) if len(t) else np.zeros(1) for t in tables]
        if len(ids0_list) != n or len(ids1_list) != n:
            raise ValueError("select_tf: one id array per side and table")
        P = ctypes.c_void_p * max(n, 1)
        ids0 = P(*[a.ctypes.data for a in keep[:n]])
        ids1 = P(*[a.ctypes.data for a in keep[n:2 * n]])
        tabs = P(*[a.ctypes.data for a in keep[2 * n:]])
        sizes = np.array([len(t) for t in tables] + [0], dtype=np.int64)
        t = self._select_terms(terms)
        m = np.ascontiguousarray(m, dtype=np.float64)
        u = np.ascontiguousarray(u, dtype=np.float64)
        k = ctypes.c_int64(0)
        check(self._lib.spk_select_tf(self._h, ctypes.c_double(lam), ctypes.c_double(one_minus), _ptr(m), _ptr(u),
                                      ctypes.c_int(n), ids0, ids1, tabs, _ptr(sizes), ctypes.c_int(len(t)),
                                      _ptr(t) if len(t) else ctypes.c_void_p(0), ctypes.byref(k)), "spk_select_tf")
        return k.value

    def select_tf_columns(self, lam, one_minus, m, u, cols, tables, terms) -> int:
        """spk_select_tf_columns: the same with the value ids taken from the device dictionary ids of the string
        columns `cols` (as tf_apply_columns)."""
        n = len(tables)
        if len(cols) != n:
            raise ValueError("select_tf_columns: one column per table")
        keep = [np.ascontiguousarray(t, dtype=np.float64) if len(t) else np.zeros(1) for t in tables]
        tabs = (ctypes.c_void_p * max(n, 1))(*[a.ctypes.data for a in keep])
        sizes = np.array([len(t) for t in tables] + [0], dtype=np.int64)
        cols = np.ascontiguousarray(list(cols) + [0], dtype=np.int32)
        t = self._select_terms(terms)
        m = np.ascontiguousarray(m, dtype=np.float64)
        u = np.ascontiguousarray(u, dtype=np.float64)
        k = ctypes.c_int64(0)
        check(self._lib.spk_select_tf_columns(self._h, ctypes.c_double(lam), ctypes.c_double(one_minus), _ptr(m), _ptr(u),
                                              ctypes.c_int(n), _ptr(cols), tabs, _ptr(sizes), ctypes.c_int(len(t)),
                                              _ptr(t) if len(t) else ctypes.c_void_p(0), ctypes.byref(k)),
              "spk_select_tf_columns")
        return k.value

    def select_copy_tf(self, start: int, count: int, n_tf: int, adj=True):
        """Survivors [start, start + count) of the last select_tf*: (tf_adjusted_match_prob, adjustments
        [count, n_tf] or None)."""
        out = np.empty(count, dtype=np.float64)
        a = np.empty((count, n_tf), dtype=np.float64) if adj else None
        check(self._lib.spk_select_copy_tf(self._h, ctypes.c_int64(start), ctypes.c_int64(count), _ptr(out), _ptr(a)),
              "spk_select_copy_tf")
        return out, a

    def select_copy(self, start: int, count: int, K: int, rows=True, gammas=True, mp=True):
        """Survivors [start, start + count) of the last select: (ordinal int64, l, r int32 or None, gammas int8
        [count, K] or None, match_probability or None)."""
        ordinal = np.empty(count, dtype=np.int64)
        l = np.empty(count, dtype=np.int32) if rows else None
        r = np.empty(count, dtype=np.int32) if rows else None
        g = np.empty((count, K), dtype=np.int8) if gammas else None
        p = np.empty(count, dtype=np.float64) if mp else None
        check(self._lib.spk_select_copy(self._h, ctypes.c_int64(start), ctypes.c_int64(count), _ptr(ordinal), _ptr(l),
                                        _ptr(r), _ptr(g), _ptr(p)), "spk_select_copy")
        return ordinal, l, r, g, p

    def select_info(self):
        """(survivors of the last select or -1, ms of its kernels with timing on or -1)."""
        n = ctypes.c_int64(-1)
        ms = ctypes.c_double(-1.0)
        check(self._lib.spk_select_info(self._h, ctypes.byref(n), ctypes.byref(ms)), "spk_select_info")
        return n.value, ms.value

    def select_release(self):
        check(self._lib.spk_select_release(self._h), "spk_select_release")

    def select_best(self, field: int, mode: int, keep_ties) -> int:
        """spk_select_best: narrow the last select to the best pair per record by `field` (SEL_MP or SEL_TF_MP) under
        `mode` (BEST_L .. BEST_MUTUAL); keep_ties: every pair at its group's maximum.  Returns how many are kept;
        they replace the selection (select_copy, select_copy_tf, select_info, components work on them)."""
        n = ctypes.c_int64(0)
        check(self._lib.spk_select_best(self._h, ctypes.c_int(int(field)), ctypes.c_int(int(mode)),
                                        ctypes.c_int(int(keep_ties)), ctypes.byref(n)), "spk_select_best")
        return n.value

    def select_best_info(self):
        """(survivors before the last select_best or -1, pairs it kept or -1, ms of its launches with timing on or -1)."""
        b = ctypes.c_int64(-1)
        k = ctypes.c_int64(-1)
        ms = ctypes.c_double(-1.0)
        check(self._lib.spk_select_best_info(self._h, ctypes.byref(b), ctypes.byref(k), ctypes.byref(ms)),
              "spk_select_best_info")
        return b.value, k.value, ms.value

    def select_sample(self, lam, one_minus, m, u, terms, edges, quota, seed) -> int:
        """spk_select_sample: per stratum of match_probability (len(edges) - 1 strata, ascending edges) keep the
        quota[b] pairs with the smallest keys of `seed` among those for which every term is TRUE; returns how many.
        They become the context's selection (select_copy, select_info, select_best, components work on them)."""
        edges = np.ascontiguousarray(edges, dtype=np.float64)
        quota = np.ascontiguousarray(quota, dtype=np.int64)
        if edges.ndim != 1 or quota.ndim != 1 or len(edges) != len(quota) + 1:
            raise ValueError("select_sample: one quota per stratum, and one edge more than strata")
        t = self._select_terms(terms)
        m = np.ascontiguousarray(m, dtype=np.float64)
        u = np.ascontiguousarray(u, dtype=np.float64)
        n = ctypes.c_int64(0)
        check(self._lib.spk_select_sample(self._h, ctypes.c_double(lam), ctypes.c_double(one_minus), _ptr(m), _ptr(u),
                                          ctypes.c_int(len(t)), _ptr(t) if len(t) else ctypes.c_void_p(0),
                                          ctypes.c_int(len(quota)), _ptr(edges),
                                          _ptr(quota) if len(quota) else ctypes.c_void_p(0),
                                          ctypes.c_uint64(int(seed)), ctypes.byref(n)), "spk_select_sample")
        return n.value

    def select_sample_info(self):
        """The last select_sample: (strata or -1, eligible pairs per stratum, pairs kept per stratum, ms of its
        launches with timing on or -1); the arrays are empty when there is none."""
        k = ctypes.c_int(-1)
        pop = np.zeros(SAMPLE_MAX_STRATA, dtype=np.int64)
        kept = np.zeros(SAMPLE_MAX_STRATA, dtype=np.int64)
        ms = ctypes.c_double(-1.0)
        check(self._lib.spk_select_sample_info(self._h, ctypes.byref(k), _ptr(pop), _ptr(kept), ctypes.byref(ms)),
              "spk_select_sample_info")
        n = max(k.value, 0)
        return k.value, pop[:n].copy(), kept[:n].copy(), ms.value

    def select_top(self, lam, one_minus, m, u, terms, order: int, k: int) -> int:
        """spk_select_top: among the pairs for which every term is TRUE keep the first k under `order` (TOP_FIRST: by
        ordinal; TOP_ASC / TOP_DESC: by match_probability, NULL lowest, ties by ordinal); returns how many.  They become
        the context's selection, in ascending ordinal.  m = u = None only with TOP_FIRST and no match_probability term."""
        t = self._select_terms(terms)
        m = None if m is None else np.ascontiguousarray(m, dtype=np.float64)
        u = None if u is None else np.ascontiguousarray(u, dtype=np.float64)
        n = ctypes.c_int64(0)
        check(self._lib.spk_select_top(self._h, ctypes.c_double(lam), ctypes.c_double(one_minus), _ptr(m), _ptr(u),
                                       ctypes.c_int(len(t)), _ptr(t) if len(t) else ctypes.c_void_p(0),
                                       ctypes.c_int(int(order)), ctypes.c_int64(int(k)), ctypes.byref(n)),
              "spk_select_top")
        return n.value

    def select_top_of(self, field: int, order: int, k: int) -> int:
        """spk_select_top_of: narrow the last select to its first k survivors under `order` by `field` (SEL_MP or
        SEL_TF_MP; ignored for TOP_FIRST).  Returns how many are kept; they replace the selection."""
        n = ctypes.c_int64(0)
        check(self._lib.spk_select_top_of(self._h, ctypes.c_int(int(field)), ctypes.c_int(int(order)),
                                          ctypes.c_int64(int(k)), ctypes.byref(n)), "spk_select_top_of")
        return n.value

    def select_top_info(self):
        """The last select_top / select_top_of: (eligible, kept, cut score, tied, tied_kept, ms).  The counts are -1 when
        there is none or it failed; the cut score is NaN without a cut (tied = 0) and for a NULL cut (tied > 0); ms is
        that of its launches with timing on, or -1."""
        e, k, t, tk = (ctypes.c_int64(-1) for _ in range(4))
        cut = ctypes.c_double(float("nan"))
        ms = ctypes.c_double(-1.0)
        check(self._lib.spk_select_top_info(self._h, ctypes.byref(e), ctypes.byref(k), ctypes.byref(cut),
                                            ctypes.byref(t), ctypes.byref(tk), ctypes.byref(ms)),
              "spk_select_top_info")
        return e.value, k.value, cut.value, t.value, tk.value, ms.value

    # ---- connected components of the kept pairs -----------------------------------------------
    def components(self):
        """spk_components over the last select's survivors: (n_nodes, n_clusters, rounds).  Node ids are input
        positions (link_only: the right table's follow the left's)."""
        n = ctypes.c_int64(0)
        c = ctypes.c_int64(0)
        r = ctypes.c_int(0)
        check(self._lib.spk_components(self._h, ctypes.byref(n), ctypes.byref(c), ctypes.byref(r)), "spk_components")
        return n.value, c.value, r.value

    def components_edges(self, n_nodes: int, u, v):
        """spk_components_edges: the same over host edges u[i] -- v[i] with ids in [0, n_nodes); returns
        (n_clusters, rounds).  An id >= n_nodes raises ValueError."""
        u = np.ascontiguousarray(u, dtype=np.uint32)
        v = np.ascontiguousarray(v, dtype=np.uint32)
        if u.shape != v.shape or u.ndim != 1:
            raise ValueError("components_edges: u and v must be one-dimensional and of one length")
        c = ctypes.c_int64(0)
        r = ctypes.c_int(0)
        check(self._lib.spk_components_edges(self._h, ctypes.c_int64(n_nodes), ctypes.c_int64(len(u)),
                                             _ptr(u) if len(u) else ctypes.c_void_p(0),
                                             _ptr(v) if len(v) else ctypes.c_void_p(0), ctypes.byref(c), ctypes.byref(r)),
              "spk_components_edges")
        return c.value, r.value

    def components_copy(self, start: int, count: int) -> np.ndarray:
        """Labels (uint32, the smallest node id of the component) of nodes [start, start + count)."""
        out = np.empty(count, dtype=np.uint32)
        check(self._lib.spk_components_copy(self._h, ctypes.c_int64(start), ctypes.c_int64(count),
                                            _ptr(out) if count else ctypes.c_void_p(0)), "spk_components_copy")
        return out

    def components_info(self):
        """(nodes, edges, rounds of the last components or -1 each, ms of its kernels with timing on or -1)."""
        n = ctypes.c_int64(-1)
        e = ctypes.c_int64(-1)
        r = ctypes.c_int(-1)
        ms = ctypes.c_double(-1.0)
        check(self._lib.spk_components_info(self._h, ctypes.byref(n), ctypes.byref(e), ctypes.byref(r), ctypes.byref(ms)),
              "spk_components_info")
        return n.value, e.value, r.value, ms.value

    def components_release(self):
        check(self._lib.spk_components_release(self._h), "spk_components_release")

    # ---- the clusters of a multi-GPU job: other ranks' labels merged in -----------------------
    @staticmethod
    def _peer_labels(peers, what="components_merge"):
        """The peers argument of components_merge / components_sweep_merge as (n_peers, address, stride, on_device,
        the object that keeps the memory alive).  peers: [n_peers, stride] (or [stride]: one peer) of uint32 / int32, a
        numpy array (or anything numpy converts) on the host, or a contiguous torch tensor on the context's device,
        which is read in place.  Needs no device: the shape, dtype and peer-count checks raise ValueError here."""
        if hasattr(peers, "is_cuda") and hasattr(peers, "data_ptr"):  # a torch tensor
            import torch
            kinds = (torch.int32,) + ((torch.uint32,) if hasattr(torch, "uint32") else ())
            if peers.dtype not in kinds:
                raise ValueError(f"{what}: peer labels are uint32 or int32, not {peers.dtype}")
            if peers.dim() == 1:
                peers = peers.unsqueeze(0)
            if peers.dim() != 2:
                raise ValueError(f"{what}: peer labels are [n_peers, stride]")
            if not 1 <= peers.shape[0] <= COMPONENTS_MAX_PEERS:
                raise ValueError(f"{what}: 1 to {COMPONENTS_MAX_PEERS} peers per call, not {peers.shape[0]}")
            if not peers.is_contiguous():
                raise ValueError(f"{what}: the peer labels must be contiguous")
            if peers.is_cuda and peers.shape[1] > 0:
                return int(peers.shape[0]), int(peers.data_ptr()), int(peers.shape[1]), True, peers
            peers = peers.cpu().numpy()  # a host tensor, or rows without nodes (no address to hand over)
        a = np.asarray(peers)
        if a.dtype not in (np.dtype(np.uint32), np.dtype(np.int32)):
            raise ValueError(f"{what}: peer labels are uint32 or int32, not {a.dtype}")
        if a.ndim == 1:
            a = a.reshape(1, -1)
        if a.ndim != 2:
            raise ValueError(f"{what}: peer labels are [n_peers, stride]")
        if not 1 <= a.shape[0] <= COMPONENTS_MAX_PEERS:
            raise ValueError(f"{what}: 1 to {COMPONENTS_MAX_PEERS} peers per call, not {a.shape[0]}")
        a = np.ascontiguousarray(a).view(np.uint32)
        if a.shape[1] == 0:  # no nodes: a non-NULL pointer the library never reads
            return int(a.shape[0]), np.zeros(1, np.uint32).ctypes.data, 0, False, a
        return int(a.shape[0]), a.ctypes.data, int(a.shape[1]), False, a

    def _settle_peers(self, on_device, keep):
        if on_device:  # written on one of torch's streams, read on the context's
            import torch
            if keep.device.index != self.device:
                raise ValueError(f"the peer labels are on {keep.device}, the context on device {self.device}")
            torch.cuda.current_stream(keep.device).synchronize()

    def components_merge(self, peers):
        """spk_components_merge: bring the labels of the last components* to those of the union of their graph with
        the graphs named by the peers' label arrays (peers[p][v] <= v: e.g. other ranks' final labels over the same
        records; `_peer_labels` for the forms).  Returns (n_clusters of the union, rounds of this call); an entry
        greater than its index raises ValueError and leaves no components.  May be called repeatedly."""
        n_peers, addr, stride, on_device, keep = self._peer_labels(peers)
        self._settle_peers(on_device, keep)
        c = ctypes.c_int64(0)
        r = ctypes.c_int(0)
        check(self._lib.spk_components_merge(self._h, ctypes.c_int(n_peers), ctypes.c_void_p(addr), ctypes.c_int64(stride),
                                             ctypes.c_int(1 if on_device else 0), ctypes.byref(c), ctypes.byref(r)),
              "spk_components_merge")
        del keep
        return c.value, r.value

    def components_copy_device(self, out, start: int = 0):
        """Labels of nodes [start, start + len(out)) of the last components* into `out`, a contiguous one-dimensional
        uint32 / int32 torch tensor on the context's device (complete on return)."""
        self._device_out(out, "components_copy_device")
        check(self._lib.spk_components_copy_device(self._h, ctypes.c_int64(start), ctypes.c_int64(out.numel()),
                                                   ctypes.c_void_p(out.data_ptr() if out.numel() else 0)),
              "spk_components_copy_device")
        return out

    def _device_out(self, out, what):
        import torch
        kinds = (torch.int32,) + ((torch.uint32,) if hasattr(torch, "uint32") else ())
        if not (out.is_cuda and out.device.index == self.device and out.dim() == 1 and out.is_contiguous()
                and out.dtype in kinds):
            raise ValueError(f"{what}: out is a contiguous one-dimensional uint32 / int32 tensor on the context's device")

    # ---- clusters at several thresholds, and their metrics ------------------------------------
    @staticmethod
    def _sweep_thresholds(thresholds):
        return np.ascontiguousarray(thresholds, dtype=np.float64).reshape(-1)  # the library validates them

    def components_sweep(self, field: int, thresholds):
        """spk_components_sweep over the last select's survivors: labels at every threshold (strictly descending) of
        the score `field` (SEL_MP, SEL_TF_MP; SEL_ALL with no thresholds: one level of every survivor).  Returns
        (n_nodes, n_edges int64 [L] cumulative, n_clusters int64 [L], rounds int32 [L])."""
        t = self._sweep_thresholds(thresholds)
        L = max(len(t), 1)
        n = ctypes.c_int64(0)
        e, c, r = np.zeros(L, dtype=np.int64), np.zeros(L, dtype=np.int64), np.zeros(L, dtype=np.int32)
        check(self._lib.spk_components_sweep(self._h, ctypes.c_int(int(field)), ctypes.c_int(len(t)),
                                             _ptr(t) if len(t) else ctypes.c_void_p(0), ctypes.byref(n), _ptr(e),
                                             _ptr(c), _ptr(r)), "spk_components_sweep")
        return n.value, e, c, r

    def components_sweep_edges(self, n_nodes: int, u, v, score, thresholds):
        """spk_components_sweep_edges: the same over host edges u[i] -- v[i] with a score each; no thresholds (score
        may be None): one level of every edge.  Returns (n_edges [L], n_clusters [L], rounds [L])."""
        u = np.ascontiguousarray(u, dtype=np.uint32)
        v = np.ascontiguousarray(v, dtype=np.uint32)
        t = self._sweep_thresholds(thresholds)
        if u.shape != v.shape or u.ndim != 1:
            raise ValueError("components_sweep_edges: u and v must be one-dimensional and of one length")
        if score is not None:
            score = np.ascontiguousarray(score, dtype=np.float64)
            if score.shape != u.shape:
                raise ValueError("components_sweep_edges: one score per edge")
        elif len(t):
            raise ValueError("components_sweep_edges: thresholds need scores")
        L = max(len(t), 1)
        e, c, r = np.zeros(L, dtype=np.int64), np.zeros(L, dtype=np.int64), np.zeros(L, dtype=np.int32)
        nul = ctypes.c_void_p(0)
        check(self._lib.spk_components_sweep_edges(
            self._h, ctypes.c_int64(n_nodes), ctypes.c_int64(len(u)), _ptr(u) if len(u) else nul,
            _ptr(v) if len(v) else nul, _ptr(score) if score is not None and len(u) else nul, ctypes.c_int(len(t)),
            _ptr(t) if len(t) else nul, _ptr(e), _ptr(c), _ptr(r)), "spk_components_sweep_edges")
        return e, c, r

    def components_sweep_copy(self, level: int, start: int, count: int) -> np.ndarray:
        """Labels (uint32) of nodes [start, start + count) at `level` of the last sweep."""
        out = np.empty(max(count, 0), dtype=np.uint32)
        check(self._lib.spk_components_sweep_copy(self._h, ctypes.c_int(level), ctypes.c_int64(start),
                                                  ctypes.c_int64(count), _ptr(out) if count > 0 else ctypes.c_void_p(0)),
              "spk_components_sweep_copy")
        return out

    def components_sweep_info(self):
        """(levels, nodes, edges of the last level of the last sweep or -1 each, ms of its kernels with timing on or -1)."""
        lv = ctypes.c_int(-1)
        n = ctypes.c_int64(-1)
        e = ctypes.c_int64(-1)
        ms = ctypes.c_double(-1.0)
        check(self._lib.spk_components_sweep_info(self._h, ctypes.byref(lv), ctypes.byref(n), ctypes.byref(e),
                                                  ctypes.byref(ms)), "spk_components_sweep_info")
        return lv.value, n.value, e.value, ms.value

    def components_sweep_release(self):
        check(self._lib.spk_components_sweep_release(self._h), "spk_components_sweep_release")

    def components_sweep_merge(self, level: int, peers):
        """spk_components_sweep_merge: components_merge on one level of the current sweep; returns (n_clusters of the
        union at that level, rounds of this call).  Marks the sweep as merged: cluster_metrics on it raises."""
        n_peers, addr, stride, on_device, keep = self._peer_labels(peers, "components_sweep_merge")
        self._settle_peers(on_device, keep)
        c = ctypes.c_int64(0)
        r = ctypes.c_int(0)
        check(self._lib.spk_components_sweep_merge(self._h, ctypes.c_int(int(level)), ctypes.c_int(n_peers),
                                                   ctypes.c_void_p(addr), ctypes.c_int64(stride),
                                                   ctypes.c_int(1 if on_device else 0), ctypes.byref(c), ctypes.byref(r)),
              "spk_components_sweep_merge")
        del keep
        return c.value, r.value

    def components_sweep_copy_device(self, level: int, out, start: int = 0):
        """components_copy_device for one level of the last sweep."""
        self._device_out(out, "components_sweep_copy_device")
        check(self._lib.spk_components_sweep_copy_device(self._h, ctypes.c_int(int(level)), ctypes.c_int64(start),
                                                         ctypes.c_int64(out.numel()),
                                                         ctypes.c_void_p(out.data_ptr() if out.numel() else 0)),
              "spk_components_sweep_copy_device")
        return out

    def components_sweep_set_mode(self, mode: int):
        """0 (default): a level hooks its new edges and a star edge per node; 1: every edge up to the level (A/B)."""
        check(self._lib.spk_components_sweep_set_mode(self._h, ctypes.c_int(int(mode))), "spk_components_sweep_set_mode")

    def cluster_metrics(self, level: int):
        """spk_cluster_metrics of one level of the last sweep: (clusters of >= 2 nodes, nodes in them, largest cluster)."""
        out = np.zeros(3, dtype=np.int64)
        check(self._lib.spk_cluster_metrics(self._h, ctypes.c_int(int(level)), _ptr(out)), "spk_cluster_metrics")
        return int(out[0]), int(out[1]), int(out[2])

    def cluster_metrics_copy(self, start: int, count: int):
        """Nodes [start, start + count) of the last cluster_metrics: (degree uint32, size uint32, degree_sum uint64,
        max_degree uint32); the last three are per cluster, at its root (label[v] == v), 0 elsewhere."""
        k = max(count, 0)
        d, s, m = np.empty(k, dtype=np.uint32), np.empty(k, dtype=np.uint32), np.empty(k, dtype=np.uint32)
        ds = np.empty(k, dtype=np.uint64)
        check(self._lib.spk_cluster_metrics_copy(self._h, ctypes.c_int64(start), ctypes.c_int64(count), _ptr(d), _ptr(s),
                                                 _ptr(ds), _ptr(m)), "spk_cluster_metrics_copy")
        return d, s, ds, m

    def cluster_metrics_set_mode(self, mode: int):
        """1 (default): the edge pass counts the lanes sharing the wave's first end; 0: one add per edge end (A/B)."""
        check(self._lib.spk_cluster_metrics_set_mode(self._h, ctypes.c_int(int(mode))), "spk_cluster_metrics_set_mode")

    def cluster_metrics_info(self):
        """(level of the last cluster_metrics or -1, ms of its kernels with timing on or -1)."""
        lv = ctypes.c_int(-1)
        ms = ctypes.c_double(-1.0)
        check(self._lib.spk_cluster_metrics_info(self._h, ctypes.byref(lv), ctypes.byref(ms)), "spk_cluster_metrics_info")
        return lv.value, ms.value

    def cluster_bridges(self, level: int):
        """spk_cluster_bridges of one level of the last sweep: (bridges, cores, nodes of the largest core, depth of the
        deepest breadth-first tree)."""
        out = np.zeros(4, dtype=np.int64)
        check(self._lib.spk_cluster_bridges(self._h, ctypes.c_int(int(level)), _ptr(out)), "spk_cluster_bridges")
        return int(out[0]), int(out[1]), int(out[2]), int(out[3])

    def cluster_bridges_copy(self, start: int, count: int):
        """Bridges [start, start + count) of the last cluster_bridges, ascending by (u, v): (u, v, side_u, side_v), uint32
        each; u -- v in the stored orientation, side_* the nodes on that end's side once the bridge is cut."""
        k = max(count, 0)
        u, v, su, sv = (np.empty(k, dtype=np.uint32) for _ in range(4))
        check(self._lib.spk_cluster_bridges_copy(self._h, ctypes.c_int64(start), ctypes.c_int64(count), _ptr(u), _ptr(v),
                                                 _ptr(su), _ptr(sv)), "spk_cluster_bridges_copy")
        return u, v, su, sv

    def cluster_bridges_cores_copy(self, start: int, count: int) -> np.ndarray:
        """core[v] (uint32) of nodes [start, start + count) of the last cluster_bridges."""
        out = np.empty(max(count, 0), dtype=np.uint32)
        check(self._lib.spk_cluster_bridges_cores_copy(self._h, ctypes.c_int64(start), ctypes.c_int64(count), _ptr(out)),
              "spk_cluster_bridges_cores_copy")
        return out

    def cluster_bridges_info(self):
        """(level of the last cluster_bridges or -1, its forest rounds or -1, ms of its kernels with timing on or -1)."""
        lv, r = ctypes.c_int(-1), ctypes.c_int(-1)
        ms = ctypes.c_double(-1.0)
        check(self._lib.spk_cluster_bridges_info(self._h, ctypes.byref(lv), ctypes.byref(r), ctypes.byref(ms)),
              "spk_cluster_bridges_info")
        return lv.value, r.value, ms.value

    # ---- pairs against labels -----------------------------------------------------------------
    def label_histogram(self, ids0, ids1=None, lam=None, one_minus=None, m=None, u=None):
        """spk_label_histogram: (counts int64 [3, n_patterns] by LABEL_NON_MATCH / LABEL_MATCH / LABEL_UNKNOWN,
        match_probability per pattern float64 [n_patterns] under lam / one_minus / m / u, or None without m / u).
        ids0 / ids1: one label id per record in device row order (negative = NULL, one id space); ids1 = None when
        the pairs' right rows index table 0."""
        ids0 = np.ascontiguousarray(ids0, dtype=np.int64)
        ids1 = None if ids1 is None else np.ascontiguousarray(ids1, dtype=np.int64)
        if (m is None) != (u is None):
            raise ValueError("label_histogram: m and u come together")
        scored = m is not None
        m = np.ascontiguousarray(m, dtype=np.float64) if scored else None
        u = np.ascontiguousarray(u, dtype=np.float64) if scored else None
        n_pat = self.n_patterns()
        counts = np.zeros((LABEL_STATES, max(n_pat, 1)), dtype=np.uint64)
        mp = np.empty(max(n_pat, 1), dtype=np.float64) if scored else None
        if ids0.size == 0:  # an empty table: a non-NULL pointer the library never reads
            ids0 = np.zeros(1, np.int64)
        if ids1 is not None and ids1.size == 0:
            ids1 = np.zeros(1, np.int64)
        check(self._lib.spk_label_histogram(self._h, _ptr(ids0), _ptr(ids1),
                                            ctypes.c_double(float(lam) if scored else 0.0),
                                            ctypes.c_double(float(one_minus) if scored else 0.0), _ptr(m), _ptr(u),
                                            _ptr(counts), _ptr(mp)), "spk_label_histogram")
        counts = counts[:, :n_pat].astype(np.int64)
        return counts, (mp[:n_pat] if scored else None)

    def label_info(self):
        """(pairs the last label_histogram counted or -1, ms of its launches with timing on or -1)."""
        n = ctypes.c_int64(-1)
        ms = ctypes.c_double(-1.0)
        check(self._lib.spk_label_info(self._h, ctypes.byref(n), ctypes.byref(ms)), "spk_label_info")
        return n.value, ms.value

    # ---- pairs against a table of labelled pairs -----------------------------------------------
    def label_pairs_histogram(self, rows_l, rows_r, is_match, lam=None, one_minus=None, m=None, u=None):
        """spk_label_pairs_histogram: (counts int64 [3, n_patterns] by LABEL_NON_MATCH / LABEL_MATCH / LABEL_UNKNOWN,
        match_probability per pattern or None without m / u, label_code int32 [n_labels]: the packed code of the
        candidate pair each label names, -1 = not among them).  rows_l / rows_r: device rows of the labelled pairs
        (in either order unless the job is link_only), is_match: 0 / 1."""
        rows_l = np.ascontiguousarray(rows_l, dtype=np.int32).reshape(-1)
        rows_r = np.ascontiguousarray(rows_r, dtype=np.int32).reshape(-1)
        is_match = np.ascontiguousarray(is_match, dtype=np.uint8).reshape(-1)
        if not len(rows_l) == len(rows_r) == len(is_match):
            raise ValueError("label_pairs_histogram: rows_l, rows_r and is_match differ in length")
        if (m is None) != (u is None):
            raise ValueError("label_pairs_histogram: m and u come together")
        scored = m is not None
        m = np.ascontiguousarray(m, dtype=np.float64) if scored else None
        u = np.ascontiguousarray(u, dtype=np.float64) if scored else None
        n, n_pat = len(rows_l), self.n_patterns()
        counts = np.zeros((LABEL_STATES, max(n_pat, 1)), dtype=np.uint64)
        mp = np.empty(max(n_pat, 1), dtype=np.float64) if scored else None
        code = np.full(max(n, 1), -1, dtype=np.int32)
        check(self._lib.spk_label_pairs_histogram(self._h, ctypes.c_int64(n), _ptr(rows_l if n else None),
                                                  _ptr(rows_r if n else None), _ptr(is_match if n else None),
                                                  ctypes.c_double(float(lam) if scored else 0.0),
                                                  ctypes.c_double(float(one_minus) if scored else 0.0), _ptr(m),
                                                  _ptr(u), _ptr(counts), _ptr(mp), _ptr(code)),
              "spk_label_pairs_histogram")
        return counts[:, :n_pat].astype(np.int64), (mp[:n_pat] if scored else None), code[:n]

    def label_pairs_info(self):
        """(pairs the last label_pairs_histogram counted, ms of its launches with timing on, slots of its hash table,
        its longest insert probe); (-1, -1.0, -1, -1): none yet, or the last call failed."""
        n, cap = ctypes.c_int64(-1), ctypes.c_int64(-1)
        ms = ctypes.c_double(-1.0)
        probe = ctypes.c_int(-1)
        check(self._lib.spk_label_pairs_info(self._h, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(cap),
                                             ctypes.byref(probe)), "spk_label_pairs_info")
        return n.value, ms.value, cap.value, probe.value

    # ---- scores against labels, per pair ------------------------------------------------------
    @staticmethod
    def _score_args(label_ids0, label_ids1, thresholds):
        """(ids0, ids1 or None, thresholds float64, zeroed counts uint64 [3, T + 2]) as the spk_label_scores_* calls
        take them; an empty id array becomes one the library never reads."""
        ids0 = np.ascontiguousarray(label_ids0, dtype=np.int64)
        ids1 = None if label_ids1 is None else np.ascontiguousarray(label_ids1, dtype=np.int64)
        if ids0.size == 0:
            ids0 = np.zeros(1, np.int64)
        if ids1 is not None and ids1.size == 0:
            ids1 = np.zeros(1, np.int64)
        t = np.ascontiguousarray(thresholds, dtype=np.float64).reshape(-1)
        return ids0, ids1, t, np.zeros((LABEL_STATES, len(t) + 2), dtype=np.uint64)

    def label_scores_tf(self, label_ids0, label_ids1, lam, one_minus, m, u, ids0_list, ids1_list, tables,
                        thresholds) -> np.ndarray:
        """spk_label_scores_tf: int64 [3, T + 2], every pair per (LABEL_* state, bin of tf_adjusted_match_prob): bin b
        in 0..T = b of the ascending `thresholds` lie below the score, bin T + 1 = a NULL score.  Label ids as for
        label_histogram, parameters, host value ids and tables as for select_tf."""
        n = len(tables)
        if len(ids0_list) != n or len(ids1_list) != n:
            raise ValueError("label_scores_tf: one id array per side and table")
        keep = [np.ascontiguousarray(a, dtype=np.int64) for a in ids0_list] + \
               [np.ascontiguousarray(a, dtype=np.int64) for a in ids1_list] + \
               [np.ascontiguousarray(t, dtype=np.float64) if len(t) else np.zeros(1) for t in tables]
        P = ctypes.c_void_p * max(n, 1)
        ids0 = P(*[a.ctypes.data for a in keep[:n]])
        ids1 = P(*[a.ctypes.data for a in keep[n:2 * n]])
        tabs = P(*[a.ctypes.data for a in keep[2 * n:]])
        sizes = np.array([len(t) for t in tables] + [0], dtype=np.int64)
        lab0, lab1, t, counts = self._score_args(label_ids0, label_ids1, thresholds)
        m = np.ascontiguousarray(m, dtype=np.float64)
        u = np.ascontiguousarray(u, dtype=np.float64)
        check(self._lib.spk_label_scores_tf(self._h, _ptr(lab0), _ptr(lab1), ctypes.c_double(lam),
                                            ctypes.c_double(one_minus), _ptr(m), _ptr(u), ctypes.c_int(n), ids0, ids1,
                                            tabs, _ptr(sizes), ctypes.c_int(len(t)),
                                            _ptr(t) if len(t) else ctypes.c_void_p(0), _ptr(counts)),
              "spk_label_scores_tf")
        return counts.astype(np.int64)

    def label_scores_tf_columns(self, label_ids0, label_ids1, lam, one_minus, m, u, cols, tables,
                                thresholds) -> np.ndarray:
        """spk_label_scores_tf_columns: the same with the value ids taken from the device dictionary ids of the string
        columns `cols` (as select_tf_columns)."""
        n = len(tables)
        if len(cols) != n:
            raise ValueError("label_scores_tf_columns: one column per table")
        keep = [np.ascontiguousarray(t, dtype=np.float64) if len(t) else np.zeros(1) for t in tables]
        tabs = (ctypes.c_void_p * max(n, 1))(*[a.ctypes.data for a in keep])
        sizes = np.array([len(t) for t in tables] + [0], dtype=np.int64)
        cols = np.ascontiguousarray(list(cols) + [0], dtype=np.int32)
        lab0, lab1, t, counts = self._score_args(label_ids0, label_ids1, thresholds)
        m = np.ascontiguousarray(m, dtype=np.float64)
        u = np.ascontiguousarray(u, dtype=np.float64)
        check(self._lib.spk_label_scores_tf_columns(self._h, _ptr(lab0), _ptr(lab1), ctypes.c_double(lam),
                                                    ctypes.c_double(one_minus), _ptr(m), _ptr(u), ctypes.c_int(n),
                                                    _ptr(cols), tabs, _ptr(sizes), ctypes.c_int(len(t)),
                                                    _ptr(t) if len(t) else ctypes.c_void_p(0), _ptr(counts)),
              "spk_label_scores_tf_columns")
        return counts.astype(np.int64)

    def label_scores_selection(self, label_ids0, label_ids1, field: int, thresholds) -> np.ndarray:
        """spk_label_scores_selection: int64 [3, T + 2] over the survivors of the last select* (or select_best), by
        `field` (SEL_MP or SEL_TF_MP); bins as for label_scores_tf."""
        lab0, lab1, t, counts = self._score_args(label_ids0, label_ids1, thresholds)
        check(self._lib.spk_label_scores_selection(self._h, _ptr(lab0), _ptr(lab1), ctypes.c_int(int(field)),
                                                   ctypes.c_int(len(t)), _ptr(t) if len(t) else ctypes.c_void_p(0),
                                                   _ptr(counts)), "spk_label_scores_selection")
        return counts.astype(np.int64)

    def label_scores_info(self):
        """(pairs the last label_scores_* counted or -1, ms of its launches with timing on or -1)."""
        n = ctypes.c_int64(-1)
        ms = ctypes.c_double(-1.0)
        check(self._lib.spk_label_scores_info(self._h, ctypes.byref(n), ctypes.byref(ms)), "spk_label_scores_info")
        return n.value, ms.value

    # ---- scores against a table of labelled pairs, per pair ------------------------------------
    @staticmethod
    def _pair_score_args(rows_l, rows_r, is_match, thresholds, what):
        """(rows_l int32, rows_r int32, is_match uint8, thresholds float64, zeroed counts uint64 [3, T + 2], label_pair
        int64 [n], label_score float64 [n]) as the spk_label_pairs_scores_* calls take them."""
        rows_l = np.ascontiguousarray(rows_l, dtype=np.int32).reshape(-1)
        rows_r = np.ascontiguousarray(rows_r, dtype=np.int32).reshape(-1)
        is_match = np.ascontiguousarray(is_match, dtype=np.uint8).reshape(-1)
        if not len(rows_l) == len(rows_r) == len(is_match):
            raise ValueError(f"{what}: rows_l, rows_r and is_match differ in length")
        t = np.ascontiguousarray(thresholds, dtype=np.float64).reshape(-1)
        n = len(rows_l)
        return (rows_l, rows_r, is_match, t, np.zeros((LABEL_STATES, len(t) + 2), dtype=np.uint64),
                np.full(max(n, 1), -1, dtype=np.int64), np.full(max(n, 1), np.nan, dtype=np.float64))

    def label_pair_scores_tf(self, rows_l, rows_r, is_match, lam, one_minus, m, u, ids0_list, ids1_list, tables,
                             thresholds):
        """spk_label_pairs_scores_tf: (counts int64 [3, T + 2]: every pair per (LABEL_* state looked up in the labelled
        pairs, bin of tf_adjusted_match_prob), label_pair int64 [n_labels]: the index of the pair each label names or
        -1, label_score float64 [n_labels]: that pair's score, NaN = none or NULL).  Labelled pairs as for
        label_pairs_histogram; parameters, host value ids, tables and bins as for label_scores_tf."""
        n = len(tables)
        if len(ids0_list) != n or len(ids1_list) != n:
            raise ValueError("label_pair_scores_tf: one id array per side and table")
        keep = [np.ascontiguousarray(a, dtype=np.int64) for a in ids0_list] + \
               [np.ascontiguousarray(a, dtype=np.int64) for a in ids1_list] + \
               [np.ascontiguousarray(t, dtype=np.float64) if len(t) else np.zeros(1) for t in tables]
        P = ctypes.c_void_p * max(n, 1)
        ids0 = P(*[a.ctypes.data for a in keep[:n]])
        ids1 = P(*[a.ctypes.data for a in keep[n:2 * n]])
        tabs = P(*[a.ctypes.data for a in keep[2 * n:]])
        sizes = np.array([len(t) for t in tables] + [0], dtype=np.int64)
        rows_l, rows_r, is_match, t, counts, pair, score = self._pair_score_args(rows_l, rows_r, is_match, thresholds,
                                                                                 "label_pair_scores_tf")
        k = len(rows_l)
        m = np.ascontiguousarray(m, dtype=np.float64)
        u = np.ascontiguousarray(u, dtype=np.float64)
        check(self._lib.spk_label_pairs_scores_tf(self._h, ctypes.c_int64(k), _ptr(rows_l if k else None),
                                                  _ptr(rows_r if k else None), _ptr(is_match if k else None),
                                                  ctypes.c_double(lam), ctypes.c_double(one_minus), _ptr(m), _ptr(u),
                                                  ctypes.c_int(n), ids0, ids1, tabs, _ptr(sizes), ctypes.c_int(len(t)),
                                                  _ptr(t) if len(t) else ctypes.c_void_p(0), _ptr(counts), _ptr(pair),
                                                  _ptr(score)), "spk_label_pairs_scores_tf")
        return counts.astype(np.int64), pair[:k], score[:k]

    def label_pair_scores_tf_columns(self, rows_l, rows_r, is_match, lam, one_minus, m, u, cols, tables, thresholds):
        """spk_label_pairs_scores_tf_columns: the same with the value ids taken from the device dictionary ids of the
        string columns `cols` (as select_tf_columns)."""
        n = len(tables)
        if len(cols) != n:
            raise ValueError("label_pair_scores_tf_columns: one column per table")
        keep = [np.ascontiguousarray(t, dtype=np.float64) if len(t) else np.zeros(1) for t in tables]
        tabs = (ctypes.c_void_p * max(n, 1))(*[a.ctypes.data for a in keep])
        sizes = np.array([len(t) for t in tables] + [0], dtype=np.int64)
        cols = np.ascontiguousarray(list(cols) + [0], dtype=np.int32)
        rows_l, rows_r, is_match, t, counts, pair, score = self._pair_score_args(rows_l, rows_r, is_match, thresholds,
                                                                                 "label_pair_scores_tf_columns")
        k = len(rows_l)
        m = np.ascontiguousarray(m, dtype=np.float64)
        u = np.ascontiguousarray(u, dtype=np.float64)
        check(self._lib.spk_label_pairs_scores_tf_columns(self._h, ctypes.c_int64(k), _ptr(rows_l if k else None),
                                                          _ptr(rows_r if k else None), _ptr(is_match if k else None),
                                                          ctypes.c_double(lam), ctypes.c_double(one_minus), _ptr(m),
                                                          _ptr(u), ctypes.c_int(n), _ptr(cols), tabs, _ptr(sizes),
                                                          ctypes.c_int(len(t)),
                                                          _ptr(t) if len(t) else ctypes.c_void_p(0), _ptr(counts),
                                                          _ptr(pair), _ptr(score)), "spk_label_pairs_scores_tf_columns")
        return counts.astype(np.int64), pair[:k], score[:k]

    def label_pair_scores_selection(self, rows_l, rows_r, is_match, field: int, thresholds):
        """spk_label_pairs_scores_selection: the same three over the survivors of the last select* (or select_best),
        by `field` (SEL_MP or SEL_TF_MP); label_pair is the survivor's index (select_copy's)."""
        rows_l, rows_r, is_match, t, counts, pair, score = self._pair_score_args(rows_l, rows_r, is_match, thresholds,
                                                                                 "label_pair_scores_selection")
        k = len(rows_l)
        check(self._lib.spk_label_pairs_scores_selection(self._h, ctypes.c_int64(k), _ptr(rows_l if k else None),
                                                         _ptr(rows_r if k else None), _ptr(is_match if k else None),
                                                         ctypes.c_int(int(field)), ctypes.c_int(len(t)),
                                                         _ptr(t) if len(t) else ctypes.c_void_p(0), _ptr(counts),
                                                         _ptr(pair), _ptr(score)), "spk_label_pairs_scores_selection")
        return counts.astype(np.int64), pair[:k], score[:k]

    def label_pair_scores_info(self):
        """(pairs the last label_pair_scores_* counted, ms of its launches with timing on, slots of its hash table, its
        longest insert probe); (-1, -1.0, -1, -1): none yet, or the last call failed."""
        n, cap = ctypes.c_int64(-1), ctypes.c_int64(-1)
        ms = ctypes.c_double(-1.0)
        probe = ctypes.c_int(-1)
        check(self._lib.spk_label_pairs_scores_info(self._h, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(cap),
                                                    ctypes.byref(probe)), "spk_label_pairs_scores_info")
        return n.value, ms.value, cap.value, probe.value

    # ---- clusters against labels --------------------------------------------------------------
    def cluster_agreement(self, ids, n_left: int = 0, cross_only: bool = False) -> np.ndarray:
        """spk_cluster_agreement: int64 [levels, AGREE_FIELDS], every level of the current sweep against one truth id
        per node (node order, negative = NULL); cross_only counts only pairs with one node below n_left."""
        ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        levels, n_nodes, _, _ = self.components_sweep_info()
        if levels >= 0 and len(ids) != n_nodes:
            raise ValueError(f"cluster_agreement: {len(ids)} ids for the sweep's {n_nodes} nodes")
        out = np.zeros((max(levels, 1), AGREE_FIELDS), dtype=np.int64)
        if ids.size == 0:  # no nodes: a non-NULL pointer the library never reads
            ids = np.zeros(1, np.int64)
        check(self._lib.spk_cluster_agreement(self._h, _ptr(ids), ctypes.c_int64(int(n_left)),
                                              ctypes.c_int(1 if cross_only else 0), _ptr(out)), "spk_cluster_agreement")
        return out

    def cluster_agreement_info(self):
        """(levels of the last cluster_agreement or -1, ms of its launches with timing on or -1)."""
        lv = ctypes.c_int(-1)
        ms = ctypes.c_double(-1.0)
        check(self._lib.spk_cluster_agreement_info(self._h, ctypes.byref(lv), ctypes.byref(ms)),
              "spk_cluster_agreement_info")
        return lv.value, ms.value

    def _udf(self, fn, left, right):
        from .table import encode_utf8
        import pandas as pd
        lo, ld, _ = encode_utf8(pd.Series(list(left), dtype=object))
        ro, rd, _ = encode_utf8(pd.Series(list(right), dtype=object))
        ld = ld if ld.size else np.zeros(1, np.uint8)
        rd = rd if rd.size else np.zeros(1, np.uint8)
        out = np.empty(len(lo) - 1, dtype=np.float64)
        check(getattr(self._lib, fn)(self._h, ctypes.c_int64(len(out)), _ptr(lo), _ptr(ld), _ptr(ro), _ptr(rd),
                                     _ptr(out)), fn)
        return out

    def jaro_winkler_sim(self, left, right):
        return self._udf("spk_jaro_winkler_sim", left, right)

    def levenshtein(self, left, right):
        return self._udf("spk_levenshtein", left, right)

    def jaccard_sim(self, left, right):
        """The jar's jaccard_sim per pair (fp64, two decimals)."""
        return self._udf("spk_jaccard_sim", left, right)

    def cosine_distance(self, left, right):
        """The jar's cosine_distance per pair (fp64); NaN where a text is blank (the reference's query fails there)."""
        return self._udf("spk_cosine_distance", left, right)

    def tf_accumulate(self, n_values, ids0, ids1):
        ids0 = np.ascontiguousarray(ids0, dtype=np.int64)
        ids1 = np.ascontiguousarray(ids1, dtype=np.int64)
        s = np.zeros(max(n_values, 1), dtype=np.float64)
        c = np.zeros(max(n_values, 1), dtype=np.int64)
        check(self._lib.spk_tf_accumulate(self._h, ctypes.c_int64(n_values), _ptr(ids0), _ptr(ids1), _ptr(s), _ptr(c)),
              "spk_tf_accumulate")
        return s[:n_values], c[:n_values]

    def tf_scales(self, n_values, ids0, ids1):
        """Per-value scales (int32: ilogb of the value's largest mp + 1) of this context's pairs; ranks
        holding shards of the pairs all-reduce them with MAX before tf_accumulate_exact."""
        ids0 = np.ascontiguousarray(ids0, dtype=np.int64)
        ids1 = np.ascontiguousarray(ids1, dtype=np.int64)
        sc = np.zeros(max(n_values, 1), dtype=np.int32)
        check(self._lib.spk_tf_scales(self._h, ctypes.c_int64(n_values), _ptr(ids0), _ptr(ids1), _ptr(sc)),
              "spk_tf_scales")
        return sc[:n_values]

    def tf_scales_column(self, col: int, n_values: int):
        sc = np.zeros(max(n_values, 1), dtype=np.int32)
        check(self._lib.spk_tf_scales_column(self._h, ctypes.c_int(col), ctypes.c_int64(n_values), _ptr(sc)),
              "spk_tf_scales_column")
        return sc[:n_values]

    def tf_accumulate_exact(self, n_values, ids0, ids1, scale):
        """Fixed-point per-value Σmp accumulators (int64 [n_values, TF_LIMBS]) relative to 2^scale, and counts:
        exact, so ranks holding shards of the pairs sum them (all-reduce) before tf_limbs_to_sum."""
        ids0 = np.ascontiguousarray(ids0, dtype=np.int64)
        ids1 = np.ascontiguousarray(ids1, dtype=np.int64)
        scale = np.ascontiguousarray(scale, dtype=np.int32)
        limbs = np.zeros((max(n_values, 1), TF_LIMBS), dtype=np.int64)
        c = np.zeros(max(n_values, 1), dtype=np.int64)
        check(self._lib.spk_tf_accumulate_exact(self._h, ctypes.c_int64(n_values), _ptr(ids0), _ptr(ids1), _ptr(scale),
                                                _ptr(limbs), _ptr(c)), "spk_tf_accumulate_exact")
        return limbs[:n_values], c[:n_values]

    def tf_accumulate_column_exact(self, col: int, n_values: int, scale):
        scale = np.ascontiguousarray(scale, dtype=np.int32)
        limbs = np.zeros((max(n_values, 1), TF_LIMBS), dtype=np.int64)
        c = np.zeros(max(n_values, 1), dtype=np.int64)
        check(self._lib.spk_tf_accumulate_column_exact(self._h, ctypes.c_int(col), ctypes.c_int64(n_values), _ptr(scale),
                                                       _ptr(limbs), _ptr(c)), "spk_tf_accumulate_column_exact")
        return limbs[:n_values], c[:n_values]

    def tf_column_values(self, col: int) -> int:
        n = ctypes.c_int64(0)
        check(self._lib.spk_tf_column_values(self._h, ctypes.c_int(col), ctypes.byref(n)), "spk_tf_column_values")
        return n.value

    def tf_accumulate_column(self, col: int, n_values: int):
        s = np.zeros(max(n_values, 1), dtype=np.float64)
        c = np.zeros(max(n_values, 1), dtype=np.int64)
        check(self._lib.spk_tf_accumulate_column(self._h, ctypes.c_int(col), ctypes.c_int64(n_values), _ptr(s), _ptr(c)),
              "spk_tf_accumulate_column")
        return s[:n_values], c[:n_values]

    def tf_apply_columns(self, cols, tables, start, count, want_adj=True, want_host=True):
        """want_host=False: tf_adjusted_match_prob stays on the device (tf_copy reads ranges of it)."""
        n = len(tables)
        keep = [np.ascontiguousarray(t, dtype=np.float64) if len(t) else np.zeros(1) for t in tables]
        tabs = (ctypes.c_void_p * n)(*[a.ctypes.data for a in keep])
        sizes = np.array([len(t) for t in tables], dtype=np.int64)
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        out = np.empty(count, dtype=np.float64) if want_host else None
        adj = np.empty((count, n), dtype=np.float64) if want_adj else None
        check(self._lib.spk_tf_apply_columns(self._h, ctypes.c_int(n), _ptr(cols), tabs, _ptr(sizes),
                                             ctypes.c_int64(start), ctypes.c_int64(count), _ptr(out), _ptr(adj)),
              "spk_tf_apply_columns")
        return out, adj

    def tf_set_mode(self, mode: int):
        check(self._lib.spk_tf_set_mode(self._h, ctypes.c_int(mode)), "spk_tf_set_mode")

    def tf_copy(self, start, count):
        out = np.empty(count, dtype=np.float64)
        check(self._lib.spk_tf_copy(self._h, ctypes.c_int64(start), ctypes.c_int64(count), _ptr(out)), "spk_tf_copy")
        return out

    def tf_apply(self, ids0_list, ids1_list, tables, start, count, want_adj=True):
        n = len(tables)
        keep = [np.ascontiguousarray(a, dtype=np.int64) for a in ids0_list] + \
               [np.ascontiguousarray(a, dtype=np.int64) for a in ids1_list] + \
               [np.ascontiguousarray(t, dtype=np.float64) if len(t) else np.zeros(1) for t in tables]
        P = ctypes.c_void_p * n
        ids0 = P(*[a.ctypes.data for a in keep[:n]])
        ids1 = P(*[a.ctypes.data for a in keep[n:2 * n]])
        tabs = P(*[a.ctypes.data for a in keep[2 * n:]])
        sizes = np.array([len(t) for t in tables], dtype=np.int64)
        out = np.empty(count, dtype=np.float64)
        adj = np.empty((count, n), dtype=np.float64) if want_adj else None
        check(self._lib.spk_tf_apply(self._h, ctypes.c_int(n), ids0, ids1, tabs, _ptr(sizes), ctypes.c_int64(start),
                                     ctypes.c_int64(count), _ptr(out), _ptr(adj)), "spk_tf_apply")
        return out, adj
