"""ctypes binding of libtantivy_amd.so: the raw C ABI (tq_*) and the C++ host mirror (tqh_*)."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libtantivy_amd.so")
if os.environ.get("TQ_LIB_PATH"):  # experiments: a variant build (tools/build_variant.py)
    LIB_PATH = os.environ["TQ_LIB_PATH"]

TERMINATED = 0x7FFFFFFF
TERM_ABSENT = 0xFFFFFFFF
TERM_ALL = 0xFFFFFFFE  # TQ_TERM_ALL: the clause is an AllQuery; accepted as a term id in every query tuple, its boost in "boosts" / weights
STAR = TERM_ALL  # what DeviceIndex.range_prepare returns in place of a handle where the range clause is an AllScorer
ALL_EMPTY, ALL_PLAIN, ALL_BASED = 0, 1, 2  # enum tq_all_kind
MODE_AND, MODE_OR, MODE_PHRASE, MODE_BOOL, MODE_TERM = 0, 1, 2, 3, 4  # enum tq_mode + TQH_MODE_TERM
SHOULD, MUST, MUST_NOT = 0, 1, 2  # src/query/occur.rs
BASIC, WITH_FREQS, WITH_FREQS_AND_POSITIONS = 0, 1, 2


class TantivyAmdError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("tantivy_amd error %d: %s" % (code, msg))
        self.code = code


class TqQuery(C.Structure):
    _fields_ = [("n_terms", C.c_uint32), ("terms", C.POINTER(C.c_uint32)),
                ("weights", C.POINTER(C.c_float)), ("tf_cache", C.POINTER(C.c_float)),
                ("mode", C.c_uint8), ("phrase_offsets", C.POINTER(C.c_uint32)),
                ("k", C.c_uint32), ("occurs", C.POINTER(C.c_uint8)),
                ("clause_of", C.POINTER(C.c_uint8)), ("min_should_match", C.c_uint32),
                ("slop", C.c_uint32),  # TQ_MODE_PHRASE: PhraseQuery::set_slop (fills what was padding: the size is unchanged)
                ("nested_occurs", C.POINTER(C.c_uint8)), ("clause_min_should", C.POINTER(C.c_uint8)),
                ("atom_of", C.POINTER(C.c_uint8))]


class TqSearchOpts(C.Structure):
    _fields_ = [("exhaustive", C.c_int32), ("bound_slack_ppm", C.c_uint32)]


OPT_DEFAULT = 0xFFFFFFFF


class TqBatchStats(C.Structure):
    _fields_ = [("algorithmic_bytes", C.c_uint64), ("matches", C.c_uint64),
                ("kernel_ms", C.c_float), ("total_ms", C.c_float), ("tiles", C.c_uint32),
                ("chunks", C.c_uint32), ("batches_averaged", C.c_uint32),
                ("host_plan_ms", C.c_float), ("kernel_mask", C.c_uint32), ("unique_bytes", C.c_uint64)]


# scan-kernel families (tq_batch_stats.kernel_mask, include/tantivy_amd.h)
KERNEL_AND_DENSE, KERNEL_AND, KERNEL_UNION, KERNEL_OR_WINDOWS, KERNEL_PHRASE = 0x1, 0x2, 0x4, 0x8, 0x10
KERNEL_PHRASE_SWEEP, KERNEL_BOOL, KERNEL_USHARE, KERNEL_XUNION, KERNEL_ASHARE = 0x20, 0x40, 0x80, 0x100, 0x200
KERNEL_BSHARE = 0x400
KERNEL_COUNT_BITMAPS = 0x800
KERNEL_TREE = 0x1000
KERNEL_DOCSET = 0x2000
KERNEL_DOCSET_SCORE = 0x4000
KERNEL_ALL = 0x8000
KERNEL_DOCSET_TREE = 0x10000
KERNEL_DOCSET_TREE_SCORE = 0x20000
KERNEL_PHRASE_SLOP = 0x40000
KERNEL_SORT = 0x80000
KERNEL_AGG = 0x100000
KERNEL_AGG_SUB = 0x200000
KERNEL_AGG_TERMS = 0x400000
KERNEL_AGG_TERMS_SUB = 0x800000
KERNEL_AGG_RANGE = 0x1000000
KERNEL_AGG_TERMS_HIST = 0x2000000
VALUE_U64, VALUE_I64, VALUE_F64 = 0, 1, 2  # tq_value_type (Bool as U64, DateTime as I64 of nanoseconds)
AGG_MAX_BUCKETS = 65536  # TQ_AGG_MAX_BUCKETS
AGG_RANGE_MAX_BUCKETS = 1024  # TQ_AGG_RANGE_MAX_BUCKETS
SORT_DESC, SORT_ASC = 0, 1      # tq_sort_order (Order::Desc = Natural, Order::Asc = ReverseNoneLower with NULLS_LAST)
NULLS_LAST, NULLS_FIRST = 0, 1  # tq_sort_nulls (NULLS_FIRST: Reverse / NaturalNoneHigher)
MAX_K = 1024  # TQ_MAX_K
MAX_SLOP, SLOP_CARRY_CAP = 255, 32  # TQ_MAX_SLOP, TQ_SLOP_CARRY_CAP (include/tantivy_amd.h "Sloppy phrases")
NESTED_PHRASE = 0x10  # tq_query.nested_occurs flag: the atom is a PhraseQuery (include/tantivy_amd.h)
KERNEL_NAMES = {0x1: "and_dense", 0x2: "and", 0x4: "union", 0x8: "or_windows", 0x10: "phrase", 0x20: "phrase_sweep",
                0x40: "bool", 0x80: "ushare", 0x100: "xunion", 0x200: "ashare", 0x400: "bshare", 0x800: "count_bitmaps",
                0x1000: "tree", 0x2000: "docset", 0x4000: "docset_score", 0x8000: "all", 0x10000: "docset_tree",
                0x20000: "docset_tree_score", 0x40000: "phrase_slop", 0x80000: "sort", 0x100000: "agg", 0x200000: "agg_sub",
                0x400000: "agg_terms", 0x800000: "agg_terms_sub", 0x1000000: "agg_range",
                0x2000000: "agg_terms_hist"}


def kernel_names(mask):
    return [n for b, n in sorted(KERNEL_NAMES.items()) if mask & b]


class TqAllForm(C.Structure):  # tq_all_form
    _fields_ = [("kind", C.c_uint32), ("base", C.c_float), ("min_should", C.c_uint32), ("keep_mask", C.c_uint32)]


class TqSubmitStats(C.Structure):
    _fields_ = [("batches", C.c_uint64), ("queries", C.c_uint64), ("max_batch", C.c_uint64)]


class TqSegmentStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        "index_bytes", "positions_bytes", "fieldnorm_bytes", "alive_bytes", "term_table_bytes",
        "bitmap_bytes", "docmat_bytes", "posdir_bytes", "scratch_bytes", "dense_budget_bytes")] + [
        (n, C.c_uint32) for n in ("n_terms", "n_dense_lists", "n_docmat_columns", "probe_evictions")] + [
        ("device_scratch_bytes", C.c_uint64), ("lead_mat_bytes", C.c_uint64), ("lead_mat_stale", C.c_uint32),
        ("pad_", C.c_uint32)]


class TqTermInfo(C.Structure):  # tq_term_info: the fields of a TermInfo as tq_term_prepare_batch takes them
    _fields_ = [("postings_off", C.c_uint64), ("positions_off", C.c_uint64), ("postings_len", C.c_uint32),
                ("positions_len", C.c_uint32), ("doc_freq", C.c_uint32), ("pad_", C.c_uint32)]


class TqFieldFiles(C.Structure):  # tq_field_files: one field's sub-files of a multi-field segment
    _fields_ = [("idx", C.c_void_p), ("idx_len", C.c_size_t), ("pos", C.c_void_p), ("pos_len", C.c_size_t),
                ("fieldnorm", C.c_void_p), ("fn_len", C.c_size_t)]


class TqFieldsStats(C.Structure):  # tq_fields_stats
    _fields_ = [("n_fields", C.c_uint32), ("n_field_terms", C.c_uint32), ("extra_fieldnorm_bytes", C.c_uint64)]


MAX_FIELDS = 8  # TQ_MAX_FIELDS


class TqhTermInfo(C.Structure):
    _fields_ = [("term_id", C.c_uint32), ("doc_freq", C.c_uint32), ("postings_start", C.c_uint64),
                ("postings_end", C.c_uint64), ("positions_start", C.c_uint64),
                ("positions_end", C.c_uint64)]


class TqhQuery(C.Structure):
    _fields_ = [("mode", C.c_uint8), ("n_terms", C.c_uint32), ("terms", C.POINTER(C.c_uint32)),
                ("phrase_offsets", C.POINTER(C.c_uint32)), ("occurs", C.POINTER(C.c_uint8)),
                ("clause_of", C.POINTER(C.c_uint8)), ("min_should_match", C.c_uint32), ("slop", C.c_uint32),
                ("boosts", C.POINTER(C.c_float)), ("nested_occurs", C.POINTER(C.c_uint8)),
                ("clause_min_should", C.POINTER(C.c_uint8)), ("atom_of", C.POINTER(C.c_uint8)),
                ("set_terms", C.POINTER(C.c_uint32)), ("set_starts", C.POINTER(C.c_uint32))]


TERM_SET_BASE = 0xFFFFFF00  # tqh_query.terms[i] == TERM_SET_BASE + j: the query's term set j (_host_queries)


class RawHandle(int):
    """A tq_term_handle as the C ABI returned it (DeviceIndex.term_set_prepare): DeviceIndex.term_handle passes it
    through untouched where a plain int is a term id of the dictionary."""


_lib = None

EXPORTS = [
    "tq_init", "tq_shutdown", "tq_last_error", "tq_segment_upload", "tq_segment_upload_device",
    "tq_segment_free",
    "tq_term_prepare", "tq_term_prepare_batch", "tq_search_batch", "tq_search_batch_device", "tq_search_batch_opts",
    "tq_search_batch_device_opts", "tq_search_batch_device_rows", "tq_merge_topk",
    "tq_merge_topk_device", "tq_copy_to_host_async", "tq_decode_postings", "tq_decode_position_deltas",
    "tq_last_batch_stats", "tq_segment_get_stats", "tq_segment_reserve_columns", "tq_set_option", "tq_segment_set_alive_bitset", "tq_count_batch",
    "tq_last_batch_match_counts", "tq_last_batch_slop_overflows", "tq_last_batch_query_kernels", "tq_encoder_create", "tq_encoder_free", "tq_encode_postings",
    "tq_encode_positions", "tq_encode_postings_device", "tq_encode_positions_device",
    "tq_encoder_last_kernel_ms", "tq_comm_unique_id", "tq_comm_init", "tq_comm_free",
    "tq_comm_info", "tq_allgather_topk",
    "tqh_last_error", "tqh_searcher_new", "tqh_searcher_free", "tqh_searcher_add_segment",
    "tqh_prepare_batch", "tqh_prepare_batch_next", "tqh_commit_next", "tqh_search_prepared", "tqh_collect_segment_prepared",
    "tqh_collect_segment_prepared_device", "tqh_search_prepared_device", "tqh_exchange_ms", "tqh_searcher_add_remote_stats",
    "tqh_bm25_for_terms", "tqh_segment_raw", "tqh_term_handle", "tqh_term_dictionary_values",
    "tqh_term_info_store_open", "tqh_term_info_store_free", "tqh_term_info_store_num_terms",
    "tqh_term_info_store_get", "tqh_term_info_store_write", "tqh_searcher_add_segment_with_store",
    "tqh_count_prepared", "tqh_searcher_add_segment_device_with_store",
    "tq_docset_batch", "tq_docset_batch_device", "tqh_docset_prepared",
    "tq_docset_scored_batch", "tq_docset_scored_batch_device", "tqh_docset_scored_prepared",
    "tq_all_query_form",
    "tq_term_set_prepare", "tq_term_set_info", "tq_term_set_release",
    "tq_segment_upload_fields", "tq_segment_get_fields_stats", "tq_term_prepare_field", "tq_term_prepare_batch_fields",
    "tq_term_field", "tqh_searcher_add_segment_fields", "tqh_searcher_add_remote_stats_fields",
    "tq_term_table_read", "tq_term_table_info",
    "tq_column_parse", "tq_column_upload", "tq_column_info", "tq_column_release", "tq_column_decode", "tq_range_prepare",
    "tq_search_sorted_batch", "tq_search_sorted_batch_device",
    "tq_agg_histogram_plan", "tq_agg_batch", "tq_agg_batch_device",
    "tq_agg_sub_batch", "tq_agg_sub_batch_device", "tq_agg_sub_lds_capacities",
    "tq_agg_terms_plan", "tq_agg_terms_batch", "tq_agg_terms_batch_device", "tq_agg_terms_lds_capacities",
    "tq_agg_terms_max_size",
    "tq_agg_terms_sub_batch", "tq_agg_terms_sub_batch_device", "tq_agg_terms_sub_lds_capacities", "tq_agg_terms_metric_image",
    "tq_agg_range_plan", "tq_agg_range_bucket_of", "tq_agg_range_batch", "tq_agg_range_batch_device",
    "tq_agg_range_lds_capacities",
    "tq_agg_terms_hist_plan", "tq_agg_terms_hist_batch", "tq_agg_terms_hist_batch_device", "tq_agg_terms_hist_lds_capacities",
]

# tq_term_table_read's tables (TQ_TABLE_*): name -> (which, dtype of the array DeviceIndex.term_table returns)
TERM_TABLES = {
    "rec": (0, np.uint32), "coarse": (1, np.uint32), "tail_docs": (2, np.uint32), "tail_tfs": (3, np.uint32),
    "pos_blk": (4, np.uint64), "pos_tail": (5, np.uint32), "dense": (6, np.uint32), "bits": (7, np.uint32),
    "pos_dir": (8, np.uint32), "tf8": (9, np.uint8), "rmax": (10, np.uint8), "rdir": (11, np.uint32),
    "lnorm": (12, np.uint8), "flat": (13, np.uint8), "probe_dense": (14, np.uint32), "probe_tf8": (15, np.uint8),
    "probe_pos_dir": (16, np.uint32), "lmat": (17, np.uint64),
    "docmat": (32, np.uint64), "doccls": (33, np.uint64), "local_cache": (34, np.float32), "min_fieldnorm_id": (35, np.uint32),
}


class TqTermTableInfo(C.Structure):  # tq_term_table_info_t
    _fields_ = [("n_blocks", C.c_uint32), ("n_full", C.c_uint32), ("n_tail", C.c_uint32), ("coarse_shift", C.c_uint32),
                ("payload_base", C.c_uint64), ("has_freq", C.c_uint32), ("rdir_shift", C.c_uint32),
                ("rmax_list", C.c_uint32), ("n_pos_blocks", C.c_uint32), ("n_pos_tail", C.c_uint32), ("field", C.c_uint32),
                ("n_positions", C.c_uint64), ("doc_freq", C.c_uint32), ("probe_slot", C.c_uint32)]


class TqColumnInfo(C.Structure):  # tq_column_info_t
    _fields_ = [("min_value", C.c_uint64), ("max_value", C.c_uint64), ("gcd", C.c_uint64), ("resident_bytes", C.c_uint64),
                ("num_rows", C.c_uint32), ("num_bits", C.c_uint32), ("codec", C.c_uint32), ("cardinality", C.c_uint32)]


MAX_COLUMNS = 16  # TQ_MAX_COLUMNS
CARD_FULL, CARD_OPTIONAL, CARD_MULTIVALUED = 0, 1, 2  # tq_cardinality
CODEC_BITPACKED, CODEC_LINEAR, CODEC_BLOCKWISE_LINEAR = 0, 1, 2  # tq_column_codec
BOUND_KINDS = {"in": 1, "ex": 2}  # tq_bound_kind (None: TQ_BOUND_UNBOUNDED)


class TqAggRequest(C.Structure):  # tq_agg_request
    _fields_ = [("column", C.c_uint32), ("value_type", C.c_uint8), ("histogram", C.c_uint8), ("has_hard_bounds", C.c_uint8),
                ("reserved", C.c_uint8), ("interval", C.c_double), ("offset", C.c_double), ("hard_min", C.c_double),
                ("hard_max", C.c_double)]


class TqAggHistPlan(C.Structure):  # tq_agg_hist_plan_t
    _fields_ = [("base_pos", C.c_int64), ("n_buckets", C.c_uint32), ("reserved", C.c_uint32), ("bounds_min", C.c_double),
                ("bounds_max", C.c_double)]


# tq_agg_stats_t as a numpy structured dtype: one 64-byte record per query
AGG_STATS_DTYPE = np.dtype([(n, np.uint64) for n in ("matches", "count", "min_value", "max_value", "sum_lo", "sum_hi",
                                                     "in_bounds", "out_of_range")])


class TqAggMetricRequest(C.Structure):  # tq_agg_metric_request
    _fields_ = [("column", C.c_uint32), ("value_type", C.c_uint8), ("reserved", C.c_uint8 * 3)]


# tq_agg_bucket_stats_t: one 40-byte record per bucket of a sub-aggregation's row
AGG_BUCKET_STATS_DTYPE = np.dtype([(n, np.uint64) for n in ("count", "min_value", "max_value", "sum_lo", "sum_hi")])


def _agg_request(column, value_type, histogram):
    """histogram: None (stats alone) or a dict with "interval" and optionally "offset" and "hard_bounds" = (min, max)."""
    req = TqAggRequest(column=int(column), value_type=int(value_type))
    if histogram is not None:
        req.histogram = 1
        req.interval = float(histogram["interval"])
        req.offset = float(histogram.get("offset", 0.0))
        hb = histogram.get("hard_bounds")
        if hb is not None:
            req.has_hard_bounds, req.hard_min, req.hard_max = 1, float(hb[0]), float(hb[1])
    return req


def agg_histogram_plan(info, value_type, interval, offset=0.0, hard_bounds=None):
    """tq_agg_histogram_plan: validation and the dense bucket range of a histogram over a column, from its info dict
    (column_parse / DeviceIndex.column_info).  -> {"base_pos", "n_buckets", "bounds_min", "bounds_max", "interval", "offset"}.
    Needs no device."""
    ci = TqColumnInfo(**{n: int(info[n]) for n, _ in TqColumnInfo._fields_ if n in info})
    req = _agg_request(0, value_type, {"interval": interval, "offset": offset, "hard_bounds": hard_bounds})
    plan = TqAggHistPlan()
    _check(lib().tq_agg_histogram_plan(C.byref(ci), C.byref(req), C.byref(plan)))
    return _agg_plan_dict(plan, req)


def _agg_plan_dict(plan, req):
    return {"base_pos": int(plan.base_pos), "n_buckets": int(plan.n_buckets), "bounds_min": float(plan.bounds_min),
            "bounds_max": float(plan.bounds_max), "interval": float(req.interval), "offset": float(req.offset)}


def agg_value_from_u64(v, value_type):
    """A u64-space value in its typed space: int for U64 / I64, float for F64 (MonotonicallyMappableToU64 inverted)."""
    v = int(v)
    if value_type == VALUE_I64:
        s = v ^ (1 << 63)
        return s - (1 << 64) if s >> 63 else s
    if value_type == VALUE_F64:
        bits = v ^ (1 << 63) if v >> 63 else v ^ ((1 << 64) - 1)
        return float(np.array([bits], np.uint64).view(np.float64)[0])
    return v


def merge_agg_stats(rows):
    """The segments' tq_agg_stats_t records of ONE query (rows of raw_agg's structured array, or dicts) as one record, a
    dict of Python ints: counts and the 128-bit sum add, min / max are the extremes.  Host only."""
    out = {"matches": 0, "count": 0, "min_value": (1 << 64) - 1, "max_value": 0, "sum": 0, "in_bounds": 0, "out_of_range": 0}
    for r in rows:
        for n in ("matches", "count", "in_bounds", "out_of_range"):
            out[n] += int(r[n])
        out["sum"] += int(r["sum_lo"]) + (int(r["sum_hi"]) << 64)
        out["min_value"] = min(out["min_value"], int(r["min_value"]))
        out["max_value"] = max(out["max_value"], int(r["max_value"]))
    out["sum_lo"], out["sum_hi"] = out["sum"] & ((1 << 64) - 1), out["sum"] >> 64
    return out


def agg_stats_finalize(stats_row, value_type):
    """IntermediateStats::finalize (stats.rs:138-161) of one record, in the typed space: {"count", "sum", "min", "max",
    "avg"}.  U64 / I64: sum is an exact Python int (I64: the u64-space sum minus count * 2^63), min / max ints, avg =
    sum / count; F64: min / max floats, sum = avg = None (not served).  count == 0: min = max = avg = None, sum 0."""
    count = int(stats_row["count"])
    if value_type == VALUE_F64:
        total = None
    else:
        total = int(stats_row["sum_lo"]) + (int(stats_row["sum_hi"]) << 64) - (count << 63 if value_type == VALUE_I64 else 0)
    if count == 0:
        return {"count": 0, "sum": total, "min": None, "max": None, "avg": None}
    return {"count": count, "sum": total, "min": agg_value_from_u64(stats_row["min_value"], value_type),
            "max": agg_value_from_u64(stats_row["max_value"], value_type), "avg": None if total is None else total / count}


def agg_sub_lds_capacities():
    """tq_agg_sub_lds_capacities: the LDS tables' capacities in buckets of agg_sub_kernel's (small, large) instantiation.
    Needs no device."""
    out = (C.c_uint32 * 2)()
    lib().tq_agg_sub_lds_capacities(out)
    return int(out[0]), int(out[1])


def merge_bucket_stats(parts):
    """The segments' bucket-record rows of ONE query and ONE request: parts = [(plan, records)] as raw_agg_sub returns them
    (plan dict, records = the query's row of AGG_BUCKET_STATS_DTYPE, or dicts).  The rows are aligned by base_pos over
    merge_histograms' range; counts and 128-bit sums add, min / max are the extremes.  -> (keys, records): records are
    dicts of Python ints like merge_agg_stats', which agg_stats_finalize takes.  Host only."""
    parts = [(p, r) for p, r in parts if p["n_buckets"]]
    if not parts:
        return [], []
    interval, offset = parts[0][0]["interval"], parts[0][0]["offset"]
    assert all(p["interval"] == interval and p["offset"] == offset for p, _ in parts)
    lo = min(p["base_pos"] for p, _ in parts)
    hi = max(p["base_pos"] + p["n_buckets"] for p, _ in parts)
    out = [{"count": 0, "min_value": (1 << 64) - 1, "max_value": 0, "sum": 0} for _ in range(hi - lo)]
    for p, recs in parts:
        for i in range(p["n_buckets"]):
            o, r = out[p["base_pos"] - lo + i], recs[i]
            o["count"] += int(r["count"])
            o["sum"] += int(r["sum_lo"]) + (int(r["sum_hi"]) << 64)
            o["min_value"] = min(o["min_value"], int(r["min_value"]))
            o["max_value"] = max(o["max_value"], int(r["max_value"]))
    for o in out:
        o["sum_lo"], o["sum_hi"] = o["sum"] & ((1 << 64) - 1), o["sum"] >> 64
    return [float(pos) * interval + offset for pos in range(lo, hi)], out


class TqAggRange(C.Structure):  # tq_agg_range_t
    _fields_ = [("from_", C.c_double), ("to", C.c_double), ("has_from", C.c_uint8), ("has_to", C.c_uint8),
                ("reserved", C.c_uint8 * 6)]


class TqAggRangeRequest(C.Structure):  # tq_agg_range_request
    _fields_ = [("column", C.c_uint32), ("value_type", C.c_uint8), ("reserved", C.c_uint8 * 3), ("n_ranges", C.c_uint32),
                ("reserved2", C.c_uint32), ("ranges", C.POINTER(TqAggRange))]


class TqAggRangeBucket(C.Structure):  # tq_agg_range_bucket_t
    _fields_ = [("start", C.c_uint64), ("end", C.c_uint64), ("source", C.c_uint32), ("reserved", C.c_uint32)]


U64_MAX = (1 << 64) - 1
RANGE_INSERTED = 0xFFFFFFFF  # tq_agg_range_bucket_t.source of a bucket the plan inserted


def _agg_range_request(column, value_type, ranges):
    """ranges: (from, to) pairs or dicts with "from" / "to"; None (or a missing key) = that end is open.  -> (request, the
    array it points to: keep it alive)."""
    arr = (TqAggRange * max(1, len(ranges)))()
    for i, r in enumerate(ranges):
        lo, hi = (r.get("from"), r.get("to")) if isinstance(r, dict) else r
        if lo is not None:
            arr[i].from_, arr[i].has_from = float(lo), 1
        if hi is not None:
            arr[i].to, arr[i].has_to = float(hi), 1
    req = TqAggRangeRequest(column=int(column), value_type=int(value_type), n_ranges=len(ranges))
    req.ranges = C.cast(arr, C.POINTER(TqAggRange))
    return req, arr


def _agg_range_plan(req):
    out = (TqAggRangeBucket * AGG_RANGE_MAX_BUCKETS)()
    n = C.c_uint32(0)
    rc = lib().tq_agg_range_plan(C.byref(req), out, AGG_RANGE_MAX_BUCKETS, C.byref(n))
    return rc, [{"start": int(b.start), "end": int(b.end), "source": None if b.source == RANGE_INSERTED else int(b.source)}
                for b in out[:n.value]]


def agg_range_plan(value_type, ranges):
    """tq_agg_range_plan: the ranges of a request as buckets [start, end) of the column's u64 space, in bucket order, the
    whole space covered (extend_validate_ranges).  ranges as for DeviceIndex.raw_agg_range.  -> a list of {"start", "end",
    "source"}: source = the index of the caller's range, None for a bucket the plan inserted.  Needs no device."""
    req, keep = _agg_range_request(0, value_type, ranges)
    rc, plan = _agg_range_plan(req)
    _check(rc)
    return plan


def agg_range_bucket_of(starts, value):
    """tq_agg_range_bucket_of: the bucket of a u64-space value among buckets with these starts — the last start <= value;
    the code the kernel runs.  Needs no device."""
    a = np.ascontiguousarray(starts, dtype=np.uint64)
    return int(lib().tq_agg_range_bucket_of(a.ctypes.data, a.size, int(value)))


def agg_range_lds_capacities():
    """tq_agg_range_lds_capacities: the record tables' capacities in buckets of agg_range_kernel's (small, large) metric
    instantiation.  Needs no device."""
    out = (C.c_uint32 * 2)()
    lib().tq_agg_range_lds_capacities(out)
    return int(out[0]), int(out[1])


def merge_ranges(parts):
    """The segments' range rows of ONE query and ONE request: parts = [(plan, counts, records or None)] as raw_agg_range
    returns them (the query's rows).  The plans must be equal (the plan depends on the request alone).  Counts add; records
    merge by merge_bucket_stats' rule.  -> (plan, counts: list of ints, records: list of dicts agg_stats_finalize takes, or
    None without a metric).  Host only."""
    plan = parts[0][0]
    assert all(p == plan for p, _, _ in parts), "the segments' plans differ"
    counts = [0] * len(plan)
    with_recs = parts[0][2] is not None
    recs = [{"count": 0, "min_value": U64_MAX, "max_value": 0, "sum": 0} for _ in plan] if with_recs else None
    for _, c, r in parts:
        for i in range(len(plan)):
            counts[i] += int(c[i])
            if with_recs:
                o = recs[i]
                o["count"] += int(r[i]["count"])
                o["sum"] += int(r[i]["sum_lo"]) + (int(r[i]["sum_hi"]) << 64)
                o["min_value"] = min(o["min_value"], int(r[i]["min_value"]))
                o["max_value"] = max(o["max_value"], int(r[i]["max_value"]))
    for o in recs or []:
        o["sum_lo"], o["sum_hi"] = o["sum"] & U64_MAX, o["sum"] >> 64
    return plan, counts, recs


def f64_display(x):
    """Rust's Display of an f64: the shortest digits that round-trip, never an exponent, no trailing ".0" ("10", "0.1",
    "-0", "1000000000000000000000", "inf", "NaN").  Python's repr has the same digits but an exponent from 1e16 on."""
    import decimal

    x = float(x)
    if x != x:
        return "NaN"
    if x in (float("inf"), float("-inf")):
        return "inf" if x > 0 else "-inf"
    t = format(decimal.Decimal(repr(x)), "f")
    return t.rstrip("0").rstrip(".") if "." in t else t


def range_key(bucket, value_type):
    """range_to_string (bucket/range.rs:521-543) of a plan's bucket for U64 / I64 / F64 columns: "*" at an open end, else
    f64_from_fastfield_u64 of the bound in Rust's Display.  DateTime keys are the caller's."""
    lo = "*" if bucket["start"] == 0 else f64_display(float(agg_value_from_u64(bucket["start"], value_type)))
    hi = "*" if bucket["end"] == U64_MAX else f64_display(float(agg_value_from_u64(bucket["end"], value_type)))
    return "%s-%s" % (lo, hi)


def range_finalize(plan, counts, records, value_type, metric_value_type=None, keys=None):
    """The final entries of one query's (merged) range rows, in bucket order: {"key", "doc_count", "from", "to"[, "stats"]}.
    from / to = f64_from_fastfield_u64(start / end), None at 0 / UINT64_MAX; key = keys[source] where the caller named the
    range (keys: a list parallel to the request's ranges, None entries allowed), else range_key; stats =
    agg_stats_finalize(record, metric_value_type) when records is given."""
    out = []
    for i, b in enumerate(plan):
        named = keys[b["source"]] if keys is not None and b["source"] is not None else None
        e = {"key": named if named is not None else range_key(b, value_type), "doc_count": int(counts[i]),
             "from": None if b["start"] == 0 else float(agg_value_from_u64(b["start"], value_type)),
             "to": None if b["end"] == U64_MAX else float(agg_value_from_u64(b["end"], value_type))}
        if records is not None:
            e["stats"] = agg_stats_finalize(records[i], metric_value_type)
        out.append(e)
    return out


class TqAggTermsRequest(C.Structure):  # tq_agg_terms_request
    _fields_ = [("column", C.c_uint32), ("order", C.c_uint32), ("segment_size", C.c_uint32)]


class TqAggTermsPlan(C.Structure):  # tq_agg_terms_plan_t
    _fields_ = [("min_value", C.c_uint64), ("gcd", C.c_uint64), ("n_keys", C.c_uint32), ("reserved", C.c_uint32)]


# tq_agg_terms_t: one 40-byte record per query of a terms aggregation
AGG_TERMS_DTYPE = np.dtype([("matches", np.uint64), ("count", np.uint64), ("sum_other_doc_count", np.uint64),
                            ("distinct", np.uint32), ("n_returned", np.uint32), ("doc_count_error_upper_bound", np.uint32),
                            ("out_of_range", np.uint32)])
TERMS_COUNT_DESC, TERMS_COUNT_ASC, TERMS_KEY_ASC, TERMS_KEY_DESC = 0, 1, 2, 3  # tq_terms_order
AGG_TERMS_MAX_SIZE = 1024  # TQ_AGG_TERMS_MAX_SIZE


def agg_terms_plan(info, order=TERMS_COUNT_DESC, segment_size=10):
    """tq_agg_terms_plan: the validation of a terms request and the key range of a column, from its info dict (column_parse /
    DeviceIndex.column_info).  -> {"n_keys", "min_value", "gcd"}; key i of a count row is min_value + gcd * i.  Needs no
    device."""
    ci = TqColumnInfo(**{n: int(info[n]) for n, _ in TqColumnInfo._fields_ if n in info})
    req = TqAggTermsRequest(column=0, order=int(order), segment_size=int(segment_size))
    plan = TqAggTermsPlan()
    _check(lib().tq_agg_terms_plan(C.byref(ci), C.byref(req), C.byref(plan)))
    return _agg_terms_plan_dict(plan)


def _agg_terms_plan_dict(plan):
    return {"n_keys": int(plan.n_keys), "min_value": int(plan.min_value), "gcd": int(plan.gcd)}


def agg_terms_lds_capacities():
    """tq_agg_terms_lds_capacities: the LDS tables' capacities in keys of agg_terms_count_kernel's (small, large)
    instantiation.  Needs no device."""
    out = (C.c_uint32 * 2)()
    lib().tq_agg_terms_lds_capacities(out)
    return int(out[0]), int(out[1])


def agg_terms_max_size():
    """tq_agg_terms_max_size: the largest segment_size a terms request may carry.  Needs no device."""
    return int(lib().tq_agg_terms_max_size())


def merge_terms(per_segment_results):
    """The segments' terms results of ONE query and ONE request as one intermediate result, as merge_fruits does for
    IntermediateTermBucketResult (intermediate_agg_result.rs:745-759): counts add per key, sum_other_doc_count and
    doc_count_error_upper_bound add.  An item is (keys, counts, record) — the query's rows and its AGG_TERMS_DTYPE record as
    raw_agg_terms returns them, of which the first n_returned entries are taken — or a dict this function returned.
    -> {"entries": {key: doc_count}, "sum_other_doc_count", "doc_count_error_upper_bound"} of Python ints.  Host only."""
    out = {"entries": {}, "sum_other_doc_count": 0, "doc_count_error_upper_bound": 0}
    for part in per_segment_results:
        if isinstance(part, dict):
            items, other, err = part["entries"].items(), part["sum_other_doc_count"], part["doc_count_error_upper_bound"]
        else:
            keys, counts, rec = part
            n = int(rec["n_returned"])
            items = zip(keys[:n], counts[:n])
            other, err = rec["sum_other_doc_count"], rec["doc_count_error_upper_bound"]
        for k, c in items:
            out["entries"][int(k)] = out["entries"].get(int(k), 0) + int(c)
        out["sum_other_doc_count"] += int(other)
        out["doc_count_error_upper_bound"] += int(err)
    return out


def terms_finalize(merged, size=10, min_doc_count=1, order=TERMS_COUNT_DESC):
    """IntermediateTermBucketResult::into_final_result (intermediate_agg_result.rs:869-961) of merge_terms' result: entries
    below min_doc_count are dropped, the rest ordered (ties of a count order by ascending key, where the reference's unstable
    sort leaves them unspecified), cut at `size`; what the cut removes is added to sum_other_doc_count, not to the error
    bound.  -> {"buckets": [(key, doc_count)], "sum_other_doc_count", "doc_count_error_upper_bound"}.  Host only."""
    entries = [(k, c) for k, c in merged["entries"].items() if c >= min_doc_count]
    if order == TERMS_COUNT_DESC:
        entries.sort(key=lambda e: (-e[1], e[0]))
    elif order == TERMS_COUNT_ASC:
        entries.sort(key=lambda e: (e[1], e[0]))
    elif order == TERMS_KEY_ASC:
        entries.sort(key=lambda e: e[0])
    elif order == TERMS_KEY_DESC:
        entries.sort(key=lambda e: -e[0])
    else:
        raise ValueError("order %r" % (order,))
    return {"buckets": entries[:size], "sum_other_doc_count": merged["sum_other_doc_count"] + sum(c for _, c in entries[size:]),
            "doc_count_error_upper_bound": merged["doc_count_error_upper_bound"]}


class TqAggTermsSubRequest(C.Structure):  # tq_agg_terms_sub_request
    _fields_ = [("column", C.c_uint32), ("order", C.c_uint32), ("segment_size", C.c_uint32), ("metric_column", C.c_uint32),
                ("metric_value_type", C.c_uint8), ("order_metric", C.c_uint8), ("reserved", C.c_uint8 * 2)]


TERMS_METRIC_DESC, TERMS_METRIC_ASC = 4, 5  # tq_terms_order, tq_agg_terms_sub_batch* alone
METRIC_VALUE_COUNT, METRIC_MIN, METRIC_MAX, METRIC_SUM, METRIC_AVG = 0, 1, 2, 3, 4  # tq_terms_metric


def agg_terms_sub_lds_capacities():
    """tq_agg_terms_sub_lds_capacities: the LDS tables' capacities in keys of agg_terms_sub_count_kernel's (small, large)
    instantiation.  Needs no device."""
    out = (C.c_uint32 * 2)()
    lib().tq_agg_terms_sub_lds_capacities(out)
    return int(out[0]), int(out[1])


def agg_terms_metric_image(record, value_type, metric):
    """tq_agg_terms_metric_image: the order value of one bucket record (a row of AGG_BUCKET_STATS_DTYPE, or a dict with
    "count", "min_value", "max_value", "sum_lo", "sum_hi") under a metric order, a Python int of up to 96 bits — the code the
    selection kernel runs, on the host.  Needs no device."""
    rec = np.zeros(1, AGG_BUCKET_STATS_DTYPE)
    for n in AGG_BUCKET_STATS_DTYPE.names:
        rec[n][0] = int(record[n])
    out = (C.c_uint64 * 2)()
    _check(lib().tq_agg_terms_metric_image(rec.ctypes.data, int(value_type), int(metric), out))
    return int(out[0]) | (int(out[1]) << 64)


def _record_dict(r):
    """A bucket record (structured row or dict) as a dict of Python ints with the 128-bit "sum"."""
    if "sum" in (r.keys() if isinstance(r, dict) else ()):
        total = int(r["sum"])
    else:
        total = int(r["sum_lo"]) + (int(r["sum_hi"]) << 64)
    return {"count": int(r["count"]), "min_value": int(r["min_value"]), "max_value": int(r["max_value"]), "sum": total,
            "sum_lo": total & ((1 << 64) - 1), "sum_hi": total >> 64}


def merge_terms_sub(per_segment_results):
    """merge_terms with a record per key: an item is (keys, counts, records, terms record) — the query's rows as
    raw_agg_terms_sub returns them, of which the first n_returned entries are taken — or a dict this function returned.
    Counts add per key as in merge_terms; the records add per key as in merge_bucket_stats (counts and 128-bit sums add, min
    / max are the extremes).  -> {"entries": {key: (doc_count, record dict)}, "sum_other_doc_count",
    "doc_count_error_upper_bound"}.  Host only."""
    out = {"entries": {}, "sum_other_doc_count": 0, "doc_count_error_upper_bound": 0}
    for part in per_segment_results:
        if isinstance(part, dict):
            items = [(k, c, r) for k, (c, r) in part["entries"].items()]
            other, err = part["sum_other_doc_count"], part["doc_count_error_upper_bound"]
        else:
            keys, counts, records, rec = part
            n = int(rec["n_returned"])
            items = zip(keys[:n], counts[:n], records[:n])
            other, err = rec["sum_other_doc_count"], rec["doc_count_error_upper_bound"]
        for k, c, r in items:
            r = _record_dict(r)
            if int(k) in out["entries"]:
                c0, r0 = out["entries"][int(k)]
                r = _record_dict({"count": r0["count"] + r["count"], "min_value": min(r0["min_value"], r["min_value"]),
                                  "max_value": max(r0["max_value"], r["max_value"]), "sum": r0["sum"] + r["sum"]})
                c = c0 + int(c)
            out["entries"][int(k)] = (int(c), r)
        out["sum_other_doc_count"] += int(other)
        out["doc_count_error_upper_bound"] += int(err)
    return out


_METRIC_FIELDS = {METRIC_VALUE_COUNT: "count", METRIC_MIN: "min", METRIC_MAX: "max", METRIC_SUM: "sum", METRIC_AVG: "avg"}


def terms_sub_finalize(merged, value_type, size=10, min_doc_count=1, order=TERMS_COUNT_DESC, order_metric=METRIC_AVG):
    """IntermediateTermBucketResult::into_final_result (intermediate_agg_result.rs:869-961) of merge_terms_sub's result.  The
    four old orders as terms_finalize; under a metric order the buckets are ordered by the finalized metric
    (agg_stats_finalize of the merged record: exact ints, avg = sum / count correctly rounded); an entry WITHOUT a metric
    value (count == 0 under min / max / avg) sorts as f64::MIN at this stage (:918-939), not as 0; ties go by ascending key.
    F64: sum / avg are not served.  -> {"buckets": [(key, doc_count, stats dict)], "sum_other_doc_count",
    "doc_count_error_upper_bound"}.  Host only."""
    entries = [(k, c, agg_stats_finalize(r, value_type)) for k, (c, r) in merged["entries"].items() if c >= min_doc_count]
    if order in (TERMS_METRIC_DESC, TERMS_METRIC_ASC):
        field = _METRIC_FIELDS[order_metric]
        if value_type == VALUE_F64 and order_metric in (METRIC_SUM, METRIC_AVG):
            raise ValueError("an order by %s of an F64 metric is not served" % field)
        f64_min = -float(np.finfo(np.float64).max)

        def val(e):
            v = e[2][field]
            return f64_min if v is None else v

        entries.sort(key=lambda e: e[0])
        entries.sort(key=val, reverse=order == TERMS_METRIC_DESC)  # (stable: ties keep the ascending key)
    elif order == TERMS_COUNT_DESC:
        entries.sort(key=lambda e: (-e[1], e[0]))
    elif order == TERMS_COUNT_ASC:
        entries.sort(key=lambda e: (e[1], e[0]))
    elif order == TERMS_KEY_ASC:
        entries.sort(key=lambda e: e[0])
    elif order == TERMS_KEY_DESC:
        entries.sort(key=lambda e: -e[0])
    else:
        raise ValueError("order %r" % (order,))
    return {"buckets": entries[:size], "sum_other_doc_count": merged["sum_other_doc_count"] + sum(e[1] for e in entries[size:]),
            "doc_count_error_upper_bound": merged["doc_count_error_upper_bound"]}


class TqAggTermsHistRequest(C.Structure):  # tq_agg_terms_hist_request
    _fields_ = [("terms", TqAggTermsRequest), ("reserved", C.c_uint32), ("hist", TqAggRequest)]


class TqAggTermsHistPlan(C.Structure):  # tq_agg_terms_hist_plan_t
    _fields_ = [("terms", TqAggTermsPlan), ("hist", TqAggHistPlan), ("n_cells", C.c_uint32), ("reserved", C.c_uint32)]


def _agg_terms_hist_request(column, hist_column, value_type, histogram, order, segment_size, reserved=(0, 0), histogram_flag=1):
    """histogram: the dict of raw_agg ("interval", optionally "offset", "hard_bounds"); reserved: the request's and the
    histogram half's reserved fields; histogram_flag: the histogram half's `histogram` byte (1 in every served request)."""
    req = TqAggTermsHistRequest()
    req.terms = TqAggTermsRequest(column=int(column), order=int(order), segment_size=int(segment_size))
    req.hist = _agg_request(hist_column, value_type, histogram)
    req.hist.histogram = int(histogram_flag)
    req.reserved, req.hist.reserved = int(reserved[0]), int(reserved[1])
    return req


def _agg_terms_hist_plan_dict(plan, req):
    return {"terms": _agg_terms_plan_dict(plan.terms), "hist": _agg_plan_dict(plan.hist, req.hist), "n_cells": int(plan.n_cells)}


def agg_terms_hist_plan(info_t, info_h, value_type, histogram, order=TERMS_COUNT_DESC, segment_size=10, reserved=(0, 0),
                        histogram_flag=1):
    """tq_agg_terms_hist_plan: the terms plan of the key column, the histogram plan of the histogram column and the grid of
    one query, from the columns' info dicts.  -> {"terms": agg_terms_plan's dict, "hist": agg_histogram_plan's dict,
    "n_cells": n_keys * (n_buckets + 1)}.  Needs no device."""
    ct = TqColumnInfo(**{n: int(info_t[n]) for n, _ in TqColumnInfo._fields_ if n in info_t})
    ch = TqColumnInfo(**{n: int(info_h[n]) for n, _ in TqColumnInfo._fields_ if n in info_h})
    req = _agg_terms_hist_request(0, 0, value_type, histogram, order, segment_size, reserved, histogram_flag)
    plan = TqAggTermsHistPlan()
    _check(lib().tq_agg_terms_hist_plan(C.byref(ct), C.byref(ch), C.byref(req), C.byref(plan)))
    return _agg_terms_hist_plan_dict(plan, req)


def agg_terms_hist_lds_capacities():
    """tq_agg_terms_hist_lds_capacities: the LDS tables' capacities in cells of agg_terms_hist_count_kernel's (small, large)
    instantiation.  Needs no device."""
    out = (C.c_uint32 * 2)()
    lib().tq_agg_terms_hist_lds_capacities(out)
    return int(out[0]), int(out[1])


def merge_terms_hist(per_segment_results):
    """merge_terms with a histogram row per key: an item is (keys, counts, rows, terms record, hist plan dict) — the query's
    rows as raw_agg_terms_hist returns them, of which the first n_returned entries are taken, and plan["hist"] of that
    segment — or a dict this function returned.  Counts add per key as in merge_terms; a key's rows are aligned by base_pos
    and added as in merge_histograms, over the dense range from the lowest to the highest bucket of ANY segment, so every
    entry carries a row of the same length.  -> {"entries": {key: (doc_count, [counts])}, "bucket_keys": [pos * interval +
    offset], "base_pos", "interval", "offset", "sum_other_doc_count", "doc_count_error_upper_bound"}.  Host only."""
    parts = []
    for part in per_segment_results:
        if isinstance(part, dict):
            if part["interval"] is None:  # (the merge of nothing)
                continue
            items = [(k, c, r) for k, (c, r) in part["entries"].items()]
            parts.append((items, part["sum_other_doc_count"], part["doc_count_error_upper_bound"], part["base_pos"],
                          len(part["bucket_keys"]), part["interval"], part["offset"]))
        else:
            keys, counts, rows, rec, hp = part
            n = int(rec["n_returned"])
            items = [(keys[j], counts[j], rows[j][:hp["n_buckets"]] if hp["n_buckets"] else []) for j in range(n)]
            parts.append((items, rec["sum_other_doc_count"], rec["doc_count_error_upper_bound"], hp["base_pos"], hp["n_buckets"],
                          hp["interval"], hp["offset"]))
    out = {"entries": {}, "bucket_keys": [], "base_pos": 0, "interval": None, "offset": None, "sum_other_doc_count": 0,
           "doc_count_error_upper_bound": 0}
    if parts:
        out["interval"], out["offset"] = parts[0][5], parts[0][6]
        assert all(p[5] == out["interval"] and p[6] == out["offset"] for p in parts)
    ranged = [p for p in parts if p[4]]
    lo = min((p[3] for p in ranged), default=0)
    hi = max((p[3] + p[4] for p in ranged), default=0)
    out["base_pos"] = lo
    out["bucket_keys"] = [float(pos) * out["interval"] + out["offset"] for pos in range(lo, hi)]
    for items, other, err, base_pos, n_buckets, _, _ in parts:
        for k, c, r in items:
            c0, row = out["entries"].get(int(k), (0, None))
            row = [0] * (hi - lo) if row is None else row
            for i in range(n_buckets):
                row[base_pos - lo + i] += int(r[i])
            out["entries"][int(k)] = (c0 + int(c), row)
        out["sum_other_doc_count"] += int(other)
        out["doc_count_error_upper_bound"] += int(err)
    return out


def terms_hist_finalize(merged, size=10, min_doc_count=1, order=TERMS_COUNT_DESC):
    """terms_finalize of merge_terms_hist's result, each bucket carrying its row: entries below min_doc_count are dropped, the
    rest ordered (ties by ascending key) and cut at `size`.  -> {"buckets": [(key, doc_count, [counts])], "bucket_keys",
    "sum_other_doc_count", "doc_count_error_upper_bound"}; a bucket's row is dense over bucket_keys (the histogram's own
    min_doc_count and extended_bounds stay the caller's).  Host only."""
    flat = terms_finalize({"entries": {k: c for k, (c, _) in merged["entries"].items()},
                           "sum_other_doc_count": merged["sum_other_doc_count"],
                           "doc_count_error_upper_bound": merged["doc_count_error_upper_bound"]}, size, min_doc_count, order)
    return {"buckets": [(k, c, list(merged["entries"][k][1])) for k, c in flat["buckets"]], "bucket_keys": list(merged["bucket_keys"]),
            "sum_other_doc_count": flat["sum_other_doc_count"], "doc_count_error_upper_bound": flat["doc_count_error_upper_bound"]}


def merge_histograms(parts):
    """The segments' histogram rows of ONE query and ONE request: parts = [(plan, counts)] as raw_agg returns them (plan
    dict, counts = the query's row).  The rows are aligned by base_pos and added.  -> (keys, counts): keys[i] = pos *
    interval + offset (get_bucket_key_from_pos) over the dense range from the lowest to the highest bucket of any segment,
    counts a list of ints.  Host only; gap filling beyond that range, min_doc_count and ordering stay the caller's."""
    parts = [(p, c) for p, c in parts if p["n_buckets"]]
    if not parts:
        return [], []
    interval, offset = parts[0][0]["interval"], parts[0][0]["offset"]
    assert all(p["interval"] == interval and p["offset"] == offset for p, _ in parts)
    lo = min(p["base_pos"] for p, _ in parts)
    hi = max(p["base_pos"] + p["n_buckets"] for p, _ in parts)
    counts = [0] * (hi - lo)
    for p, c in parts:
        for i in range(p["n_buckets"]):
            counts[p["base_pos"] - lo + i] += int(c[i])
    return [float(pos) * interval + offset for pos in range(lo, hi)], counts


def _column_info_dict(info):
    return {n: int(getattr(info, n)) for n, _ in TqColumnInfo._fields_}


def column_parse(values_bytes):
    """tq_column_parse: the host-side check of one serialized u64_based column-values blob -> dict of tq_column_info_t
    (codec, min_value, max_value, gcd, num_rows, num_bits, resident_bytes).  Needs no device."""
    a = np.frombuffer(bytes(values_bytes) + b"\0", dtype=np.uint8)  # (an empty blob is still a pointer)
    info = TqColumnInfo()
    _check(lib().tq_column_parse(a.ctypes.data, a.size - 1, C.byref(info)))
    return _column_info_dict(info)


def lib():
    """Loads the HIP library.  No fallback: a missing library is an error."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise TantivyAmdError(-1, "%s not built (run `python -m tantivy_amd.build` or "
                                  "__graft_entry__.build())" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, u8p, u32p, f32p = C.c_void_p, C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_float)
    L.tq_last_error.restype = C.c_char_p
    L.tqh_last_error.restype = C.c_char_p
    L.tq_init.argtypes = [C.POINTER(C.c_int), C.c_int, C.POINTER(vp)]
    L.tq_shutdown.argtypes = [vp]
    L.tq_segment_upload.argtypes = [vp, C.c_int, C.c_uint32, vp, C.c_size_t, vp, C.c_size_t, vp,
                                    C.c_size_t, C.c_uint8, C.POINTER(vp)]
    L.tq_segment_upload_device.argtypes = [vp, C.c_int, C.c_uint32, vp, C.c_size_t, vp, C.c_size_t, vp,
                                           C.c_size_t, C.c_uint8, C.POINTER(vp)]
    L.tq_segment_free.argtypes = [vp]
    L.tq_term_prepare.argtypes = [vp, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32,
                                  u32p]
    L.tq_term_prepare_batch.argtypes = [vp, C.POINTER(TqTermInfo), C.c_uint32, u32p]
    L.tq_search_batch.argtypes = [vp, C.POINTER(TqQuery), C.c_uint32, C.c_uint32, f32p, u32p, u32p]
    L.tq_search_batch_device.argtypes = [vp, C.POINTER(TqQuery), C.c_uint32, C.c_uint32, vp, vp,
                                         vp, vp]
    L.tq_search_batch_opts.argtypes = [vp, C.POINTER(TqQuery), C.c_uint32, C.c_uint32, f32p, u32p,
                                       u32p, C.POINTER(TqSearchOpts)]
    L.tq_search_batch_device_opts.argtypes = [vp, C.POINTER(TqQuery), C.c_uint32, C.c_uint32, vp,
                                              vp, vp, C.POINTER(TqSearchOpts), vp]
    L.tq_search_batch_device_rows.argtypes = [vp, C.POINTER(TqQuery), C.c_uint32, C.c_uint32, vp, vp,
                                              vp, vp, C.c_uint32, C.POINTER(TqSearchOpts), vp]
    L.tq_merge_topk.argtypes = [f32p, u32p, u32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                C.c_uint32, f32p, u32p, u32p, u32p]
    L.tq_copy_to_host_async.argtypes = [vp, C.c_int, vp, vp, C.c_size_t, vp]
    L.tq_merge_topk_device.argtypes = [vp, C.c_int, vp, vp, vp, vp, C.c_uint32, C.c_uint32,
                                       C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp]
    L.tq_decode_postings.argtypes = [vp, C.c_uint32, u32p, u32p]
    L.tq_decode_position_deltas.argtypes = [vp, C.c_uint32, u32p, C.c_uint64,
                                            C.POINTER(C.c_uint64)]
    L.tq_last_batch_stats.argtypes = [vp, C.POINTER(TqBatchStats)]
    L.tq_segment_get_stats.argtypes = [vp, C.POINTER(TqSegmentStats)]
    L.tq_segment_reserve_columns.argtypes = [vp, C.POINTER(C.c_uint64), C.c_uint32]
    L.tq_set_option.argtypes = [vp, C.c_char_p, C.c_int64]
    L.tq_segment_set_alive_bitset.argtypes = [vp, vp, C.c_size_t]
    L.tq_count_batch.argtypes = [vp, C.POINTER(TqQuery), C.c_uint32, u32p]
    L.tq_last_batch_match_counts.argtypes = [vp, u32p, C.c_uint32]
    L.tq_last_batch_slop_overflows.argtypes = [vp, u32p, C.c_uint32]
    L.tq_docset_batch.argtypes = [vp, C.POINTER(TqQuery), C.c_uint32, u32p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.tq_docset_batch_device.argtypes = [vp, C.POINTER(TqQuery), C.c_uint32, vp, C.c_uint64, vp, vp]
    L.tqh_docset_prepared.argtypes = [vp, u32p, u32p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.tq_docset_scored_batch.argtypes = [vp, C.POINTER(TqQuery), C.c_uint32, u32p, f32p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.tq_docset_scored_batch_device.argtypes = [vp, C.POINTER(TqQuery), C.c_uint32, vp, vp, C.c_uint64, vp, vp]
    L.tqh_docset_scored_prepared.argtypes = [vp, u32p, u32p, f32p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.tq_last_batch_query_kernels.argtypes = [vp, u32p, C.c_uint32]
    L.tq_all_query_form.argtypes = [C.POINTER(TqQuery), C.POINTER(TqAllForm)]
    L.tq_term_set_prepare.argtypes = [vp, u32p, C.c_uint32, u32p]
    L.tq_term_set_info.argtypes = [vp, C.c_uint32, u32p, C.POINTER(C.c_uint64)]
    L.tq_term_set_release.argtypes = [vp, C.c_uint32]
    L.tq_segment_upload_fields.argtypes = [vp, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(TqFieldFiles), C.c_uint8, C.POINTER(vp)]
    L.tq_segment_get_fields_stats.argtypes = [vp, C.POINTER(TqFieldsStats)]
    L.tq_term_prepare_field.argtypes = [vp, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, u32p]
    L.tq_term_prepare_batch_fields.argtypes = [vp, C.POINTER(TqTermInfo), u8p, C.c_uint32, u32p]
    L.tq_term_field.argtypes = [vp, C.c_uint32, u32p]
    L.tq_term_table_read.argtypes = [vp, C.c_uint32, C.c_uint32, vp, C.c_uint64, C.POINTER(C.c_uint64)]
    L.tq_term_table_info.argtypes = [vp, C.c_uint32, C.POINTER(TqTermTableInfo)]
    L.tq_column_parse.argtypes = [vp, C.c_size_t, C.POINTER(TqColumnInfo)]
    L.tq_column_upload.argtypes = [vp, vp, C.c_size_t, C.c_uint8, u32p, u32p]
    L.tq_column_info.argtypes = [vp, C.c_uint32, C.POINTER(TqColumnInfo)]
    L.tq_column_release.argtypes = [vp, C.c_uint32]
    L.tq_column_decode.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
    L.tq_range_prepare.argtypes = [vp, C.c_uint32, C.c_uint8, C.c_uint64, C.c_uint8, C.c_uint64, C.c_float, u32p, f32p]
    L.tq_search_sorted_batch.argtypes = [vp, C.POINTER(TqQuery), C.c_uint32, C.c_uint32, C.c_uint8, C.c_uint8, C.c_uint32,
                                         u32p, C.POINTER(C.c_uint64), u8p, u32p]
    L.tq_search_sorted_batch_device.argtypes = [vp, C.POINTER(TqQuery), C.c_uint32, C.c_uint32, C.c_uint8, C.c_uint8, C.c_uint32,
                                                vp, vp, vp, vp, vp]
    L.tq_agg_histogram_plan.argtypes = [C.POINTER(TqColumnInfo), C.POINTER(TqAggRequest), C.POINTER(TqAggHistPlan)]
    L.tq_agg_batch.argtypes = [vp, C.POINTER(TqQuery), C.c_uint32, C.POINTER(TqAggRequest), vp, u32p, C.c_uint32]
    L.tq_agg_batch_device.argtypes = [vp, C.POINTER(TqQuery), C.c_uint32, C.POINTER(TqAggRequest), vp, vp, C.c_uint32, vp]
    L.tq_agg_sub_batch.argtypes = [vp, C.POINTER(TqQuery), C.c_uint32, C.POINTER(TqAggRequest), C.POINTER(TqAggMetricRequest),
                                   vp, u32p, vp, C.c_uint32]
    L.tq_agg_sub_batch_device.argtypes = [vp, C.POINTER(TqQuery), C.c_uint32, C.POINTER(TqAggRequest),
                                          C.POINTER(TqAggMetricRequest), vp, vp, vp, C.c_uint32, vp]
    L.tq_agg_sub_lds_capacities.argtypes = [C.POINTER(C.c_uint32)]
    L.tq_agg_sub_lds_capacities.restype = None
    L.tq_agg_terms_plan.argtypes = [C.POINTER(TqColumnInfo), C.POINTER(TqAggTermsRequest), C.POINTER(TqAggTermsPlan)]
    L.tq_agg_terms_batch.argtypes = [vp, C.POINTER(TqQuery), C.c_uint32, C.POINTER(TqAggTermsRequest), vp, vp, u32p, C.c_uint32]
    L.tq_agg_terms_batch_device.argtypes = [vp, C.POINTER(TqQuery), C.c_uint32, C.POINTER(TqAggTermsRequest), vp, vp, vp,
                                            C.c_uint32, vp]
    L.tq_agg_terms_lds_capacities.argtypes = [C.POINTER(C.c_uint32)]
    L.tq_agg_terms_lds_capacities.restype = None
    L.tq_agg_terms_sub_batch.argtypes = [vp, C.POINTER(TqQuery), C.c_uint32, C.POINTER(TqAggTermsSubRequest), vp, vp, u32p, vp,
                                         C.c_uint32]
    L.tq_agg_terms_sub_batch_device.argtypes = [vp, C.POINTER(TqQuery), C.c_uint32, C.POINTER(TqAggTermsSubRequest), vp, vp, vp, vp,
                                                C.c_uint32, vp]
    L.tq_agg_terms_sub_lds_capacities.argtypes = [C.POINTER(C.c_uint32)]
    L.tq_agg_terms_sub_lds_capacities.restype = None
    L.tq_agg_terms_metric_image.argtypes = [vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
    L.tq_agg_range_plan.argtypes = [C.POINTER(TqAggRangeRequest), C.POINTER(TqAggRangeBucket), C.c_uint32, u32p]
    L.tq_agg_range_bucket_of.argtypes = [vp, C.c_uint32, C.c_uint64]
    L.tq_agg_range_bucket_of.restype = C.c_uint32
    L.tq_agg_range_batch.argtypes = [vp, C.POINTER(TqQuery), C.c_uint32, C.POINTER(TqAggRangeRequest),
                                     C.POINTER(TqAggMetricRequest), vp, u32p, vp, C.c_uint32]
    L.tq_agg_range_batch_device.argtypes = [vp, C.POINTER(TqQuery), C.c_uint32, C.POINTER(TqAggRangeRequest),
                                            C.POINTER(TqAggMetricRequest), vp, vp, vp, C.c_uint32, vp]
    L.tq_agg_range_lds_capacities.argtypes = [C.POINTER(C.c_uint32)]
    L.tq_agg_range_lds_capacities.restype = None
    L.tq_agg_terms_hist_plan.argtypes = [C.POINTER(TqColumnInfo), C.POINTER(TqColumnInfo), C.POINTER(TqAggTermsHistRequest),
                                         C.POINTER(TqAggTermsHistPlan)]
    L.tq_agg_terms_hist_batch.argtypes = [vp, C.POINTER(TqQuery), C.c_uint32, C.POINTER(TqAggTermsHistRequest), vp, vp, u32p, u32p,
                                          C.c_uint32, C.c_uint32]
    L.tq_agg_terms_hist_batch_device.argtypes = [vp, C.POINTER(TqQuery), C.c_uint32, C.POINTER(TqAggTermsHistRequest), vp, vp, vp, vp,
                                                 C.c_uint32, C.c_uint32, vp]
    L.tq_agg_terms_hist_lds_capacities.argtypes = [C.POINTER(C.c_uint32)]
    L.tq_agg_terms_hist_lds_capacities.restype = None
    L.tq_agg_terms_max_size.argtypes = []
    L.tq_agg_terms_max_size.restype = C.c_uint32
    L.tqh_searcher_add_segment_fields.argtypes = [vp, C.c_int, C.c_uint32, C.c_uint8, C.c_uint32, C.POINTER(TqFieldFiles),
                                                  C.POINTER(TqhTermInfo), u8p, C.c_uint32]
    L.tqh_searcher_add_remote_stats_fields.argtypes = [vp, C.c_uint64, C.POINTER(C.c_uint64), C.c_uint32, u32p, u32p, C.c_uint32]
    u64p = C.POINTER(C.c_uint64)
    L.tq_encoder_create.argtypes = [vp, C.c_int, C.POINTER(vp)]
    L.tq_encoder_free.argtypes = [vp]
    L.tq_encoder_free.restype = None
    L.tq_encode_postings.argtypes = [vp, C.c_uint32, vp, vp, vp, vp, C.c_uint32, C.c_float,
                                     C.c_uint8, vp, C.c_uint64, vp, u64p]
    L.tq_encode_positions.argtypes = [vp, C.c_uint32, vp, vp, vp, C.c_uint64, vp, u64p]
    L.tq_encode_postings_device.argtypes = [vp, C.c_uint32, vp, vp, vp, vp, vp, C.c_uint32,
                                            C.c_float, C.c_uint8, vp, C.c_uint64, vp, u64p, vp]
    L.tq_encode_positions_device.argtypes = [vp, C.c_uint32, vp, vp, vp, vp, C.c_uint64, vp, u64p,
                                             vp]
    L.tq_encoder_last_kernel_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.tq_comm_unique_id.argtypes = [vp]
    L.tq_comm_init.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.POINTER(vp)]
    L.tq_comm_free.argtypes = [vp]
    L.tq_comm_free.restype = None
    L.tq_comm_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_char_p)]
    L.tq_allgather_topk.argtypes = [vp, vp, vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp]
    L.tqh_searcher_new.argtypes = [vp, C.POINTER(vp)]
    L.tqh_searcher_free.argtypes = [vp]
    L.tqh_searcher_add_segment.argtypes = [vp, C.c_int, C.c_uint32, C.c_uint8, vp, C.c_size_t, vp,
                                           C.c_size_t, vp, C.c_size_t, C.POINTER(TqhTermInfo),
                                           C.c_uint32]
    L.tqh_prepare_batch.argtypes = [vp, C.POINTER(TqhQuery), C.c_uint32]
    L.tqh_prepare_batch_next.argtypes = [vp, C.POINTER(TqhQuery), C.c_uint32]
    L.tqh_commit_next.argtypes = [vp]
    L.tqh_search_prepared.argtypes = [vp, C.c_uint32, C.c_uint32, f32p, u32p, u32p, u32p]
    L.tqh_search_concurrent.argtypes = [vp, C.POINTER(TqhQuery), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                        f32p, u32p, u32p, u32p, f32p, C.POINTER(C.c_double)]
    L.tq_get_submit_stats.argtypes = [vp, C.POINTER(TqSubmitStats), C.c_int]
    L.tq_search_one.argtypes = [vp, C.POINTER(TqQuery), C.POINTER(TqSearchOpts), f32p, u32p, u32p]
    L.tq_submit.argtypes = [vp, C.POINTER(TqQuery), C.POINTER(TqSearchOpts), f32p, u32p, u32p, C.POINTER(vp)]
    L.tq_wait.argtypes = [vp]
    L.tqh_collect_segment_prepared.argtypes = [vp, C.c_uint32, C.c_uint32, f32p, u32p, u32p]
    L.tqh_collect_segment_prepared_device.argtypes = [vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp]
    L.tqh_search_prepared_device.argtypes = [vp, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.tqh_exchange_ms.argtypes = [vp, f32p]
    L.tqh_searcher_add_remote_stats.argtypes = [vp, C.c_uint64, C.c_uint64, u32p, u32p, C.c_uint32]
    L.tqh_bm25_for_terms.argtypes = [C.POINTER(C.c_uint64), C.c_uint32, C.c_uint64, C.c_uint64,
                                     C.c_float, f32p, f32p]
    L.tqh_segment_raw.restype = vp
    L.tqh_segment_raw.argtypes = [vp, C.c_uint32]
    L.tqh_term_handle.restype = C.c_uint32
    L.tqh_term_handle.argtypes = [vp, C.c_uint32, C.c_uint32]
    L.tqh_term_dictionary_values.argtypes = [vp, C.c_size_t, u64p, u64p]
    L.tqh_count_prepared.argtypes = [vp, u64p]
    L.tqh_term_info_store_open.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
    L.tqh_term_info_store_free.argtypes = [vp]
    L.tqh_term_info_store_free.restype = None
    L.tqh_term_info_store_num_terms.argtypes = [vp]
    L.tqh_term_info_store_num_terms.restype = C.c_uint64
    L.tqh_term_info_store_get.argtypes = [vp, vp, C.c_uint32, C.POINTER(TqhTermInfo)]
    L.tqh_term_info_store_write.argtypes = [C.POINTER(TqhTermInfo), C.c_uint32, vp, C.c_uint64, u64p]
    L.tqh_searcher_add_segment_with_store.argtypes = [vp, C.c_int, C.c_uint32, C.c_uint8, vp,
                                                      C.c_size_t, vp, C.c_size_t, vp, C.c_size_t,
                                                      vp, C.c_size_t]
    L.tqh_searcher_add_segment_device_with_store.argtypes = [
        vp, C.c_int, C.c_uint32, C.c_uint8, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t,
        C.c_uint64, vp, C.c_size_t]
    _lib = L
    return L


def _check(rc, host=False):
    if rc != 0:
        L = lib()
        msg = (L.tqh_last_error() if host else L.tq_last_error()) or b""
        if host and not msg:
            msg = L.tq_last_error() or b""
        raise TantivyAmdError(rc, msg.decode("utf-8", "replace"))


def _f32(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _u32(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def bm25_for_terms(doc_freqs, total_num_docs, total_num_tokens, boost=1.0):
    """Product-side Bm25Weight::for_terms: returns (weight, cache[256]) of ONE field's statistics; the tf_cache of a
    multi-field segment is np.stack of one such cache per field (total_num_tokens = that field's)."""
    dfs = (C.c_uint64 * len(doc_freqs))(*[int(d) for d in doc_freqs])
    w = C.c_float()
    cache = np.zeros(256, np.float32)
    _check(lib().tqh_bm25_for_terms(dfs, len(doc_freqs), int(total_num_docs), int(total_num_tokens),
                                    C.c_float(boost), C.byref(w), _f32(cache)), host=True)
    return float(w.value), cache


def all_query_form(handles, weights=None, mode=MODE_BOOL, occurs=None, clause_of=None, min_should_match=0):
    """tq_all_query_form: the normal form of a query with TERM_ALL clauses -> (rc, kind, base, min_should, keep_mask).
    handles: term HANDLES (TERM_ALL, TERM_ABSENT, anything else counts as a present list); weights None = NULL."""
    n = len(handles)
    q = TqQuery()
    hs = (C.c_uint32 * max(1, n))(*[int(h) for h in handles])
    q.n_terms, q.terms, q.mode, q.k = n, C.cast(hs, C.POINTER(C.c_uint32)), int(mode), 1
    q.min_should_match = int(min_should_match)
    keep = [hs]
    if weights is not None:
        ws = (C.c_float * max(1, n))(*[float(w) for w in weights])
        keep.append(ws)
        q.weights = C.cast(ws, C.POINTER(C.c_float))
    if occurs is not None:
        oc = (C.c_uint8 * max(1, n))(*[int(o) for o in occurs])
        keep.append(oc)
        q.occurs = C.cast(oc, C.POINTER(C.c_uint8))
    if clause_of is not None:
        co = (C.c_uint8 * max(1, n))(*[int(o) for o in clause_of])
        keep.append(co)
        q.clause_of = C.cast(co, C.POINTER(C.c_uint8))
    f = TqAllForm()
    rc = lib().tq_all_query_form(C.byref(q), C.byref(f))
    return rc, int(f.kind), float(f.base), int(f.min_should), int(f.keep_mask)


def sort_key(value, has_value, order, nulls):
    """The (class, value') part of the sorted calls' key, in Python ints; SMALLER sorts first.  value' is the value for
    SORT_ASC and its complement for SORT_DESC; docs without a value after (NULLS_LAST) or before (NULLS_FIRST) the others."""
    if not has_value:
        return (0 if nulls == NULLS_FIRST else 2, 0)
    v = int(value)
    return (1, v if order == SORT_ASC else (1 << 64) - 1 - v)


def merge_sorted_top_k(rows_per_segment, k, order, nulls, offset=0):
    """The reference's merge_top_k (src/collector/top_score_collector.rs) over the segments' sorted rows of ONE query:
    rows_per_segment[segment_ord] = (docs, values, has_value, count) as raw_search_sorted returns a row.  The merged order is
    the comparator on Option<u64>, ties by ascending (segment_ord, doc); -> the entries [offset, offset + k) as a list of
    (value or None, segment_ord, doc).  Host only."""
    entries = []
    for seg_ord, (docs, values, has_value, count) in enumerate(rows_per_segment):
        for i in range(int(count)):
            has = bool(has_value[i])
            entries.append((sort_key(values[i], has, order, nulls), seg_ord, int(docs[i]), int(values[i]) if has else None))
    entries.sort(key=lambda e: e[:3])
    return [(v, s, d) for _, s, d, v in entries[int(offset): int(offset) + int(k)]]


def term_dictionary_values(field_file):
    """(offset, length) of the TermInfoStore inside a field's term dictionary file."""
    b = np.frombuffer(bytes(field_file), dtype=np.uint8)
    off, ln = C.c_uint64(), C.c_uint64()
    _check(lib().tqh_term_dictionary_values(b.ctypes.data, b.size, C.byref(off), C.byref(ln)), host=True)
    return int(off.value), int(ln.value)


class TermInfoStore:
    """Host-side TermInfoStore (tantivy_amd/host/term_info_store.hpp)."""

    def __init__(self, store_bytes):
        b = np.frombuffer(bytes(store_bytes), dtype=np.uint8)
        self._h = C.c_void_p()
        _check(lib().tqh_term_info_store_open(b.ctypes.data, b.size, C.byref(self._h)), host=True)

    def num_terms(self):
        return int(lib().tqh_term_info_store_num_terms(self._h))

    def get(self, ords):
        """[(doc_freq, postings_start, postings_end, positions_start, positions_end), ...]"""
        o = np.ascontiguousarray(ords, np.uint64)
        out = (TqhTermInfo * max(1, o.size))()
        _check(lib().tqh_term_info_store_get(self._h, o.ctypes.data, o.size, out), host=True)
        return [(t.doc_freq, t.postings_start, t.postings_end, t.positions_start, t.positions_end)
                for t in out[: o.size]]

    def close(self):
        if self._h:
            lib().tqh_term_info_store_free(self._h)
            self._h = None

    @staticmethod
    def serialize(term_infos):
        """TermInfoStoreWriter over (doc_freq, ps, pe, qs, qe) tuples in ordinal order."""
        n = len(term_infos)
        tis = (TqhTermInfo * max(1, n))()
        for i, t in enumerate(term_infos):
            tis[i] = TqhTermInfo(i, *[int(x) for x in t])
        need = C.c_uint64()
        out = np.zeros(64 + 48 * n, np.uint8)
        rc = lib().tqh_term_info_store_write(tis, n, out.ctypes.data, out.size, C.byref(need))
        if rc != 0 and need.value > out.size:
            out = np.zeros(need.value, np.uint8)
            rc = lib().tqh_term_info_store_write(tis, n, out.ctypes.data, out.size, C.byref(need))
        _check(rc, host=True)
        return out[: need.value].tobytes()


class Encoder:
    """Device-side PostingsSerializer / PositionSerializer (tq_encode_*), host buffers in and out."""

    def __init__(self, device=0):
        self._ctx = C.c_void_p()
        arr = (C.c_int * 1)(device)
        _check(lib().tq_init(arr, 1, C.byref(self._ctx)))
        self._e = C.c_void_p()
        _check(lib().tq_encoder_create(self._ctx, device, C.byref(self._e)))

    def close(self):
        if self._e:
            lib().tq_encoder_free(self._e)
            self._e = None
        if self._ctx:
            lib().tq_shutdown(self._ctx)
            self._ctx = None

    def _run(self, call, n_terms, est):
        out = np.zeros(max(16, est), np.uint8)
        ots = np.zeros(n_terms + 1, np.uint64)
        need = C.c_uint64()
        rc = call(out, ots, need)
        if rc != 0 and need.value > out.size:  # too small: the call reported the size
            out = np.zeros(need.value, np.uint8)
            rc = call(out, ots, need)
        _check(rc)
        return out[: need.value].copy(), ots

    def encode_postings(self, term_starts, docs, tfs, fieldnorm_ids, num_docs, avg_fieldnorm,
                        record_option, out_cap=None):
        ts = np.ascontiguousarray(term_starts, np.uint64)
        docs = np.ascontiguousarray(docs, np.uint32)
        tfs = None if tfs is None else np.ascontiguousarray(tfs, np.uint32)
        fn = None if fieldnorm_ids is None else np.ascontiguousarray(fieldnorm_ids, np.uint8)

        def call(out, ots, need):
            return lib().tq_encode_postings(
                self._e, len(ts) - 1, ts.ctypes.data, docs.ctypes.data,
                None if tfs is None else tfs.ctypes.data, None if fn is None else fn.ctypes.data,
                int(num_docs), C.c_float(avg_fieldnorm), int(record_option), out.ctypes.data,
                out.size, ots.ctypes.data, C.byref(need))

        est = out_cap if out_cap is not None else int(docs.size) * 3 + 64 * len(ts)
        return self._run(call, len(ts) - 1, est)

    def encode_positions(self, term_starts, deltas, out_cap=None):
        ts = np.ascontiguousarray(term_starts, np.uint64)
        deltas = np.ascontiguousarray(deltas, np.uint32)

        def call(out, ots, need):
            return lib().tq_encode_positions(self._e, len(ts) - 1, ts.ctypes.data,
                                             deltas.ctypes.data, out.ctypes.data, out.size,
                                             ots.ctypes.data, C.byref(need))

        est = out_cap if out_cap is not None else int(deltas.size) * 2 + 64 * len(ts)
        return self._run(call, len(ts) - 1, est)

    def last_kernel_ms(self):
        ms = C.c_float()
        _check(lib().tq_encoder_last_kernel_ms(self._e, C.byref(ms)))
        return float(ms.value)

    @property
    def raw(self):
        return self._e


class DeviceIndex:
    """A Searcher over device-resident segments (C++ host mirror, tantivy_amd/host/searcher.hpp).

    segments: iterable of objects with max_doc, record_option, idx (np.uint8, header included),
    pos, fieldnorm (or None) and terms: list of (doc_freq, postings_start, postings_end,
    positions_start, positions_end); term id = list index.
    """

    def __init__(self, segments=(), devices=None):
        L = lib()
        self._ctx = C.c_void_p()
        devs = list(devices) if devices is not None else [0]
        arr = (C.c_int * len(devs))(*devs)
        _check(L.tq_init(arr, len(devs), C.byref(self._ctx)))
        self._s = C.c_void_p()
        _check(L.tqh_searcher_new(self._ctx, C.byref(self._s)), host=True)
        self._devs = devs
        self.n_segments = 0
        self._keep = []
        self._n_prepared = 0
        for i, seg in enumerate(segments):
            self.add_segment(seg, devs[i % len(devs)])

    def add_segment(self, seg, device=0, term_info_store=None):
        """term_info_store: the bytes of the segment's TermInfoStore; then term ids are term
        ordinals and seg.terms is not consulted (TermInfos are decoded by the library)."""
        L = lib()
        idx = np.ascontiguousarray(seg.idx[: seg.idx_len] if hasattr(seg, "idx_len") else seg.idx,
                                   dtype=np.uint8)
        pos_len = getattr(seg, "pos_len", len(seg.pos) if seg.pos is not None else 0)
        pos = np.ascontiguousarray(seg.pos[:pos_len], dtype=np.uint8) if pos_len else None
        fn = None if seg.fieldnorm is None else np.ascontiguousarray(seg.fieldnorm, dtype=np.uint8)
        if term_info_store is not None:
            st = np.frombuffer(bytes(term_info_store), dtype=np.uint8)
            _check(L.tqh_searcher_add_segment_with_store(
                self._s, int(device), int(seg.max_doc), int(seg.record_option),
                idx.ctypes.data, idx.size, pos.ctypes.data if pos is not None else None,
                pos.size if pos is not None else 0, fn.ctypes.data if fn is not None else None,
                fn.size if fn is not None else 0, st.ctypes.data, st.size), host=True)
            self.n_segments += 1
            return
        n = len(seg.terms)
        tis = (TqhTermInfo * max(1, n))()
        for i, t in enumerate(seg.terms):
            if isinstance(t, (tuple, list)):
                df, ps, pe, qs, qe = t
            else:
                df, ps, pe, qs, qe = (t.doc_freq, t.postings_start, t.postings_end,
                                      t.positions_start, t.positions_end)
            tis[i] = TqhTermInfo(i, int(df), int(ps), int(pe), int(qs), int(qe))
        _check(L.tqh_searcher_add_segment(
            self._s, int(device), int(seg.max_doc), int(seg.record_option),
            idx.ctypes.data, idx.size, pos.ctypes.data if pos is not None else None,
            pos.size if pos is not None else 0, fn.ctypes.data if fn is not None else None,
            fn.size if fn is not None else 0, tis, n), host=True)
        self.n_segments += 1

    def add_segment_fields(self, fields, device=0):
        """One segment of several fields over one doc-id space (tq_segment_upload_fields).  fields: a list of objects
        shaped like add_segment's segment objects (idx with its header, pos, fieldnorm or None, terms), one per field,
        sharing max_doc and record_option; fields[0] is the primary field.  TERM IDS ARE ASSIGNED FIELD BY FIELD IN
        ORDER: field 0's terms get 0 .. len(fields[0].terms) - 1, field 1's the next len(fields[1].terms), and so on
        (field_term_base(fields, f) + the term's index in fields[f].terms).  Queries name these ids as on a single-field
        segment; every term scores under its own field's fieldnorms and average fieldnorm.  -> the term-id base of
        every field."""
        L = lib()
        if not 1 <= len(fields) <= MAX_FIELDS:
            raise TantivyAmdError(1, "add_segment_fields: %d fields, 1..%d are taken" % (len(fields), MAX_FIELDS))
        if any(f.max_doc != fields[0].max_doc or f.record_option != fields[0].record_option for f in fields):
            raise TantivyAmdError(1, "add_segment_fields: the fields of a segment share max_doc and record_option")
        ff = (TqFieldFiles * len(fields))()
        keep, tis_list, tfs, bases = [], [], [], []
        for f, seg in enumerate(fields):
            idx = np.ascontiguousarray(seg.idx[: seg.idx_len] if hasattr(seg, "idx_len") else seg.idx, dtype=np.uint8)
            pos_len = getattr(seg, "pos_len", len(seg.pos) if seg.pos is not None else 0)
            pos = np.ascontiguousarray(seg.pos[:pos_len], dtype=np.uint8) if pos_len else None
            fn = None if seg.fieldnorm is None else np.ascontiguousarray(seg.fieldnorm, dtype=np.uint8)
            keep += [idx, pos, fn]
            ff[f] = TqFieldFiles(idx.ctypes.data, idx.size, pos.ctypes.data if pos is not None else None,
                                 pos.size if pos is not None else 0, fn.ctypes.data if fn is not None else None,
                                 fn.size if fn is not None else 0)
            bases.append(len(tis_list))
            for t in seg.terms:
                if isinstance(t, (tuple, list)):
                    df, ps, pe, qs, qe = t
                else:
                    df, ps, pe, qs, qe = (t.doc_freq, t.postings_start, t.postings_end, t.positions_start, t.positions_end)
                tis_list.append(TqhTermInfo(len(tis_list), int(df), int(ps), int(pe), int(qs), int(qe)))
                tfs.append(f)
        n = len(tis_list)
        tis = (TqhTermInfo * max(1, n))(*tis_list)
        tfa = (C.c_uint8 * max(1, n))(*tfs)
        _check(L.tqh_searcher_add_segment_fields(self._s, int(device), int(fields[0].max_doc), int(fields[0].record_option),
                                                 len(fields), ff, tis, tfa, n), host=True)
        self.n_segments += 1
        return bases

    def add_remote_stats_fields(self, max_doc, total_num_tokens_per_field, doc_freqs):
        """add_remote_stats for multi-field segments: one token count per field; doc_freqs indexed by term id."""
        toks = (C.c_uint64 * len(total_num_tokens_per_field))(*[int(t) for t in total_num_tokens_per_field])
        ids = np.arange(len(doc_freqs), dtype=np.uint32)
        dfs = np.ascontiguousarray(doc_freqs, dtype=np.uint32)
        _check(lib().tqh_searcher_add_remote_stats_fields(self._s, int(max_doc), toks, len(total_num_tokens_per_field),
                                                          _u32(ids), _u32(dfs), len(dfs)), host=True)

    def add_segment_device(self, max_doc, record_option, d_idx, d_pos, d_fieldnorm,
                           total_num_tokens, term_info_store, device=0):
        """Segment whose sub-files are torch uint8 tensors on the GPU (d_idx with the 8-byte
        header; d_pos / d_fieldnorm may be None); term ids = ordinals of term_info_store."""
        st = np.frombuffer(bytes(term_info_store), dtype=np.uint8)
        _check(lib().tqh_searcher_add_segment_device_with_store(
            self._s, int(device), int(max_doc), int(record_option), d_idx.data_ptr(), d_idx.numel(),
            d_pos.data_ptr() if d_pos is not None else None,
            d_pos.numel() if d_pos is not None else 0,
            d_fieldnorm.data_ptr() if d_fieldnorm is not None else None,
            d_fieldnorm.numel() if d_fieldnorm is not None else 0, int(total_num_tokens),
            st.ctypes.data, st.size), host=True)
        self.n_segments += 1

    def add_remote_stats(self, max_doc, total_num_tokens, doc_freqs):
        """doc_freqs: sequence indexed by term id (segments held by other ranks)."""
        ids = np.arange(len(doc_freqs), dtype=np.uint32)
        dfs = np.ascontiguousarray(doc_freqs, dtype=np.uint32)
        _check(lib().tqh_searcher_add_remote_stats(self._s, int(max_doc), int(total_num_tokens),
                                                   _u32(ids), _u32(dfs), len(dfs)), host=True)

    def close(self):
        L = lib()
        if getattr(self, "_prep_pool", None) is not None:
            self._prep_pool.shutdown(wait=True)
            self._prep_pool = None
        if self._s:
            L.tqh_searcher_free(self._s)
            self._s = C.c_void_p()
        if self._ctx:
            L.tq_shutdown(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- host-mirror path (Query::weight + Searcher::search)
    def _host_queries(self, queries):
        """-> (tqh_query array, keep-alive list).  queries: list of (mode, [term ids]), (MODE_PHRASE, [term ids], [offsets]
        [, slop]) — PhraseQuery::set_slop, include/tantivy_amd.h "Sloppy phrases" — or
        (MODE_BOOL, [term ids], [occurs][, clause_of | None[, min_should_match]]) with occurs in
        {SHOULD, MUST, MUST_NOT}; terms sharing a clause_of value form one nested union.  A trailing
        dict {"boosts": [...]} wraps every term query in BoostQuery(boost); {"nested_occurs": [...]}
        gives the occur of every term INSIDE its clause_of group (255 = Should: a nested union), e.g.
        `+a +(+b -c)` = (MODE_BOOL, [a, b, c], [MUST]*3, [0, 1, 1], 0, {"nested_occurs": [255, 1, 2]}).  A phrase
        inside a boolean query: its terms share an "atom_of" value, carry nested_occurs | NESTED_PHRASE and their
        "phrase_offsets" — `+"a b" +c` = (MODE_BOOL, [a, b, c], [MUST]*3, [0, 0, 1], 0, {"nested_occurs": [0x11, 0x11, 1],
        "atom_of": [0, 0, 0], "phrase_offsets": [0, 1, 0]}).  A TERM SET (Query::term_set: a TermSetQuery, or the terms a
        fuzzy / regex automaton matched) stands in the term list as a tuple ("set", [term ids]) in place of a term id —
        `+a +set(x y z)` = (MODE_AND, [a, ("set", [x, y, z])]); its entry of "boosts" is the score of every doc of the set."""
        n = len(queries)
        qs = (TqhQuery * max(1, n))()
        keep = []
        for i, q in enumerate(queries):
            extra = q[-1] if isinstance(q[-1], dict) else None
            if extra is not None:
                q = q[:-1]
            mode, terms = q[0], list(q[1])
            if any(isinstance(t, tuple) for t in terms):  # term sets: ("set", [term ids]) -> TERM_SET_BASE + j
                members, starts = [], [0]
                for j, t in enumerate(terms):
                    if isinstance(t, tuple):
                        assert t[0] == "set", t
                        members += [int(x) for x in t[1]]
                        terms[j] = TERM_SET_BASE + len(starts) - 1
                        starts.append(len(members))
                sm = (C.c_uint32 * max(1, len(members)))(*members)
                ss = (C.c_uint32 * len(starts))(*starts)
                keep += [sm, ss]
                qs[i].set_terms = C.cast(sm, C.POINTER(C.c_uint32))
                qs[i].set_starts = C.cast(ss, C.POINTER(C.c_uint32))
            if extra and extra.get("boosts") is not None:
                ba = (C.c_float * len(terms))(*[float(b) for b in extra["boosts"]])
                keep.append(ba)
                qs[i].boosts = C.cast(ba, C.POINTER(C.c_float))
            if extra and extra.get("nested_occurs") is not None:
                na = (C.c_uint8 * len(terms))(*[int(o) for o in extra["nested_occurs"]])
                keep.append(na)
                qs[i].nested_occurs = C.cast(na, C.POINTER(C.c_uint8))
            if extra and extra.get("atom_of") is not None:
                aa = (C.c_uint8 * len(terms))(*[int(o) for o in extra["atom_of"]])
                keep.append(aa)
                qs[i].atom_of = C.cast(aa, C.POINTER(C.c_uint8))
            if extra and extra.get("phrase_offsets") is not None:  # MODE_BOOL: offsets of the terms of phrases inside it
                pa = (C.c_uint32 * len(terms))(*[int(o) for o in extra["phrase_offsets"]])
                keep.append(pa)
                qs[i].phrase_offsets = C.cast(pa, C.POINTER(C.c_uint32))
            if extra and extra.get("clause_min_should") is not None:  # {clause_of value: nested minimum}
                ma = (C.c_uint8 * 16)(*[int(extra["clause_min_should"].get(c, 0)) for c in range(16)])
                keep.append(ma)
                qs[i].clause_min_should = C.cast(ma, C.POINTER(C.c_uint8))
            ta = (C.c_uint32 * len(terms))(*[int(t) for t in terms])
            keep.append(ta)
            qs[i].mode = mode
            qs[i].n_terms = len(terms)
            qs[i].terms = C.cast(ta, C.POINTER(C.c_uint32))
            if mode == MODE_BOOL:
                oc = (C.c_uint8 * len(terms))(*[int(o) for o in q[2]])
                keep.append(oc)
                qs[i].occurs = C.cast(oc, C.POINTER(C.c_uint8))
                if len(q) > 3 and q[3] is not None:
                    co = (C.c_uint8 * len(terms))(*[int(o) for o in q[3]])
                    keep.append(co)
                    qs[i].clause_of = C.cast(co, C.POINTER(C.c_uint8))
                if len(q) > 4:
                    qs[i].min_should_match = int(q[4])
            elif len(q) > 2 and q[2] is not None:
                oa = (C.c_uint32 * len(terms))(*[int(o) for o in q[2]])
                keep.append(oa)
                qs[i].phrase_offsets = C.cast(oa, C.POINTER(C.c_uint32))
            if mode == MODE_PHRASE and len(q) > 3:  # (MODE_PHRASE, [ids], [offsets] | None, slop)
                qs[i].slop = int(q[3])
        return qs, keep

    def prepare(self, queries):
        """Query::weight for a batch (see _host_queries for the query tuples)."""
        self.prepare_marshalled(self.marshal(queries))

    def marshal(self, queries):
        """The query tuples of a batch as the C structs tqh_prepare_batch takes (the Python side of a caller's
        request decoding: done ahead of a timed region that is to hold Query::weight itself)."""
        qs, keep = self._host_queries(queries)
        return qs, keep, len(queries)

    def prepare_marshalled(self, m):
        """Query::weight (+ tq_term_prepare and first-use tables of terms not seen before) for a marshalled batch."""
        qs, _, n = m
        _check(lib().tqh_prepare_batch(self._s, qs, n), host=True)
        self._n_prepared = n

    def prepare_next_async(self, m):
        """Query::weight of the NEXT batch on a helper thread (ctypes drops the GIL for the call) while this thread
        executes the current one; commit_next() waits for it and makes it the current batch.  Returns nothing: one
        batch can be in preparation at a time."""
        import concurrent.futures

        if getattr(self, "_prep_pool", None) is None:
            # the helper keeps off the caller's physical core: woken by the caller, the scheduler likes to put it on the
            # SMT sibling of the caller's CPU, where the two halve each other (Query::weight for 10 000 queries: 0.65 ms
            # alone, 2.5 ms on the sibling of a planning thread)
            avoid = set()
            try:
                cpu = os.sched_getcpu()
                with open("/sys/devices/system/cpu/cpu%d/topology/thread_siblings_list" % cpu) as f:
                    for part in f.read().strip().split(","):
                        lo, _, hi = part.partition("-")
                        avoid.update(range(int(lo), int(hi or lo) + 1))
            except (OSError, ValueError, AttributeError):
                avoid = set()

            def keep_off():
                try:
                    allowed = os.sched_getaffinity(0) - avoid
                    if allowed:
                        os.sched_setaffinity(0, allowed)
                except (OSError, AttributeError):
                    pass

            self._prep_pool = concurrent.futures.ThreadPoolExecutor(max_workers=1, initializer=keep_off)
        qs, _, n = m

        def work():
            import time as _t

            t0 = _t.perf_counter()
            _check(lib().tqh_prepare_batch_next(self._s, qs, n), host=True)
            return _t.perf_counter() - t0

        self._prep_next = (self._prep_pool.submit(work), n, m)

    def commit_next(self):
        """-> seconds the preparation took on its thread."""
        fut, n, _ = self._prep_next
        secs = fut.result()
        self._prep_next = None
        _check(lib().tqh_commit_next(self._s), host=True)
        self._n_prepared = n
        return secs

    def search_concurrent(self, queries, limit, n_threads, offset=0):
        """Searcher::search from n_threads host threads at once, one query per call (tantivy's own call
        pattern): the per-segment calls of concurrent threads are coalesced into batched launches
        (tq_search_one).  Returns (scores, segment_ords, docs, counts, latency_ms per query, wall_ms)."""
        qs, keep = self._host_queries(queries)
        n = len(queries)
        scores = np.zeros((n, limit), np.float32)
        ords = np.zeros((n, limit), np.uint32)
        docs = np.zeros((n, limit), np.uint32)
        counts = np.zeros(n, np.uint32)
        lat = np.zeros(max(1, n), np.float32)
        wall = C.c_double()
        _check(lib().tqh_search_concurrent(self._s, qs, n, int(offset), int(limit), int(n_threads),
                                           _f32(scores), _u32(ords), _u32(docs), _u32(counts), _f32(lat),
                                           C.byref(wall)), host=True)
        return scores, ords, docs, counts, lat[:n], float(wall.value)

    def submit_stats(self, segment_ord=0, reset=False):
        """Launches issued for queries that came through tq_submit / tq_search_one on one segment."""
        st = TqSubmitStats()
        _check(lib().tq_get_submit_stats(self.segment_raw(segment_ord), C.byref(st), 1 if reset else 0))
        return {"batches": int(st.batches), "queries": int(st.queries), "max_batch": int(st.max_batch)}

    def search_prepared(self, limit, offset=0):
        n = self._n_prepared
        scores = np.zeros((n, limit), np.float32)
        ords = np.zeros((n, limit), np.uint32)
        docs = np.zeros((n, limit), np.uint32)
        counts = np.zeros(n, np.uint32)
        _check(lib().tqh_search_prepared(self._s, int(offset), int(limit), _f32(scores),
                                         _u32(ords), _u32(docs), _u32(counts)), host=True)
        return scores, ords, docs, counts

    def collect_segment_prepared(self, segment_ord, k):
        n = self._n_prepared
        scores = np.zeros((n, k), np.float32)
        docs = np.zeros((n, k), np.uint32)
        counts = np.zeros(n, np.uint32)
        _check(lib().tqh_collect_segment_prepared(self._s, int(segment_ord), int(k), _f32(scores),
                                                  _u32(docs), _u32(counts)), host=True)
        return scores, docs, counts

    def collect_segment_prepared_device(self, segment_ord, k, d_scores, d_docs, d_counts,
                                        stream=None):
        """torch tensors (float32 [n,k], int32 [n,k], int32 [n]) on the segment's GPU."""
        _check(lib().tqh_collect_segment_prepared_device(
            self._s, int(segment_ord), int(k), d_scores.data_ptr(), d_docs.data_ptr(),
            d_counts.data_ptr(), C.c_void_p(stream) if stream else None), host=True)

    def search_prepared_device(self, k, out, slabs=None, stream=None):
        """Searcher::search of the prepared batch, limit k, as one native call that only enqueues work on `stream`
        (tqh_search_prepared_device).  out = (scores float32 [n,k], segment ordinals, docs int32 [n,k], counts int32 [n]):
        torch tensors on the segments' GPU or in pinned host memory; slabs = ([S*n,k] float32, [S*n,k] int32, [S*n] int32)
        device tensors, needed with several segments."""
        sl = [t.data_ptr() for t in slabs] if slabs is not None else [None, None, None]
        _check(lib().tqh_search_prepared_device(
            self._s, int(k), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(),
            sl[0], sl[1], sl[2], C.c_void_p(stream) if stream else None), host=True)

    def exchange_ms(self):
        """Mean GPU time of the merge_top_k launches of the last (<= 16) search_prepared_device calls; 0.0 with one segment."""
        ms = C.c_float(0.0)
        _check(lib().tqh_exchange_ms(self._s, C.byref(ms)), host=True)
        return float(ms.value)

    @property
    def ctx(self):
        return self._ctx

    def search(self, queries, limit, offset=0):
        self.prepare(queries)
        return self.search_prepared(limit, offset)

    def count(self, queries):
        """Searcher::search(&query, &Count) for a batch: alive matching docs over all segments."""
        self.prepare(queries)
        out = np.zeros(max(1, len(queries)), np.uint64)
        _check(lib().tqh_count_prepared(self._s, out.ctypes.data_as(C.POINTER(C.c_uint64))), host=True)
        return out[: len(queries)]

    def docset(self, queries):
        """Searcher::search(&query, &DocSetCollector) for a batch: per query an (n, 2) uint32 array of
        (segment_ord, doc) rows — the alive matching docs of every segment, ordered by (segment_ord, doc)."""
        self.prepare(queries)
        n = len(queries)
        starts = np.zeros(n + 1, np.uint64)
        ords = np.zeros(1, np.uint32)
        docs = np.zeros(1, np.uint32)
        u64p = C.POINTER(C.c_uint64)
        rc = lib().tqh_docset_prepared(self._s, _u32(ords), _u32(docs), 0, starts.ctypes.data_as(u64p))
        if rc != 0 and int(starts[n]) > 0:  # too small: the call reported the size
            ords = np.zeros(int(starts[n]), np.uint32)
            docs = np.zeros(int(starts[n]), np.uint32)
            rc = lib().tqh_docset_prepared(self._s, _u32(ords), _u32(docs), docs.size, starts.ctypes.data_as(u64p))
        _check(rc, host=True)
        pairs = np.stack([ords, docs], axis=1)
        return [pairs[int(starts[q]): int(starts[q + 1])] for q in range(n)]

    def docset_scored(self, queries):
        """Searcher::search with a collector that needs scores (Weight::for_each) for a batch: per query the (n, 2)
        uint32 array of (segment_ord, doc) rows docset() returns and a float32 array of their BM25 scores under the
        index-wide statistics."""
        self.prepare(queries)
        n = len(queries)
        starts = np.zeros(n + 1, np.uint64)
        ords = np.zeros(1, np.uint32)
        docs = np.zeros(1, np.uint32)
        scores = np.zeros(1, np.float32)
        u64p = C.POINTER(C.c_uint64)
        rc = lib().tqh_docset_scored_prepared(self._s, _u32(ords), _u32(docs), _f32(scores), 0, starts.ctypes.data_as(u64p))
        if rc != 0 and int(starts[n]) > 0:  # too small: the call reported the size
            ords = np.zeros(int(starts[n]), np.uint32)
            docs = np.zeros(int(starts[n]), np.uint32)
            scores = np.zeros(int(starts[n]), np.float32)
            rc = lib().tqh_docset_scored_prepared(self._s, _u32(ords), _u32(docs), _f32(scores), docs.size,
                                                  starts.ctypes.data_as(u64p))
        _check(rc, host=True)
        pairs = np.stack([ords, docs], axis=1)
        return [(pairs[int(starts[q]): int(starts[q + 1])], scores[int(starts[q]): int(starts[q + 1])]) for q in range(n)]

    # ---- raw C ABI access (parity tests)
    def segment_raw(self, segment_ord=0):
        return C.c_void_p(lib().tqh_segment_raw(self._s, segment_ord))

    def term_handle(self, term_id, segment_ord=0):
        if isinstance(term_id, RawHandle):  # (a handle already: a term set of term_set_prepare)
            return int(term_id)
        if int(term_id) == TERM_ALL:  # (an AllQuery clause names no list: the value is its own handle)
            return TERM_ALL
        return lib().tqh_term_handle(self._s, segment_ord, int(term_id))

    def term_field(self, handle, segment_ord=0):
        """tq_term_field: the field of a multi-field segment the HANDLE's list belongs to (0: the primary field)."""
        f = C.c_uint32()
        _check(lib().tq_term_field(self.segment_raw(segment_ord), int(handle), C.byref(f)))
        return int(f.value)

    def fields_stats(self, segment_ord=0):
        """tq_segment_get_fields_stats -> {n_fields, n_field_terms, extra_fieldnorm_bytes}."""
        st = TqFieldsStats()
        _check(lib().tq_segment_get_fields_stats(self.segment_raw(segment_ord), C.byref(st)))
        return {"n_fields": int(st.n_fields), "n_field_terms": int(st.n_field_terms),
                "extra_fieldnorm_bytes": int(st.extra_fieldnorm_bytes)}

    def term_set_prepare(self, term_ids, segment_ord=0):
        """tq_term_set_prepare on one segment: the OR of the docs of the terms `term_ids` (ids of the term dictionary, or
        RawHandles / TERM_ABSENT as they are) as a const-scoring list -> RawHandle, which every raw_* helper takes in its
        term lists in place of a term id."""
        hs = np.array([self.term_handle(t, segment_ord) for t in term_ids], np.uint32)
        out = C.c_uint32()
        _check(lib().tq_term_set_prepare(self.segment_raw(segment_ord), _u32(hs) if hs.size else None, int(hs.size), C.byref(out)))
        return RawHandle(out.value)

    def term_set_info(self, h, segment_ord=0):
        """tq_term_set_info -> (docs in the set, resident bytes)."""
        n_docs, nbytes = C.c_uint32(), C.c_uint64()
        _check(lib().tq_term_set_info(self.segment_raw(segment_ord), int(h), C.byref(n_docs), C.byref(nbytes)))
        return int(n_docs.value), int(nbytes.value)

    def term_set_release(self, h, segment_ord=0):
        _check(lib().tq_term_set_release(self.segment_raw(segment_ord), int(h)))

    # ---- fast-field columns and range clauses (tq_column.cpp, tq_range.hip)
    def add_column(self, values_bytes, cardinality=CARD_FULL, present=None, segment_ord=0):
        """tq_column_upload on one segment: `values_bytes` = one serialized u64_based column-values blob; `present` (for
        CARD_OPTIONAL) = ceil(max_doc / 32) uint32 words, bit d set when doc d has a value.  -> the column's index."""
        a = np.frombuffer(bytes(values_bytes) + b"\0", dtype=np.uint8)
        words = None if present is None else np.ascontiguousarray(present, dtype=np.uint32)
        out = C.c_uint32()
        _check(lib().tq_column_upload(self.segment_raw(segment_ord), a.ctypes.data, a.size - 1, int(cardinality),
                                      _u32(words) if words is not None else None, C.byref(out)))
        return int(out.value)

    def column_info(self, column, segment_ord=0):
        """tq_column_info -> dict of tq_column_info_t."""
        info = TqColumnInfo()
        _check(lib().tq_column_info(self.segment_raw(segment_ord), int(column), C.byref(info)))
        return _column_info_dict(info)

    def column_release(self, column, segment_ord=0):
        _check(lib().tq_column_release(self.segment_raw(segment_ord), int(column)))

    def column_decode(self, column, first_row=0, n=None, segment_ord=0):
        """tq_column_decode: the values of rows [first_row, first_row + n) (default: to the last row) as uint64."""
        if n is None:
            n = self.column_info(column, segment_ord)["num_rows"] - first_row
        out = np.zeros(max(1, int(n)), np.uint64)
        _check(lib().tq_column_decode(self.segment_raw(segment_ord), int(column), int(first_row), int(n),
                                      out.ctypes.data_as(C.POINTER(C.c_uint64))))
        return out[: int(n)]

    def range_prepare(self, column, lower, upper, boost=1.0, segment_ord=0):
        """tq_range_prepare: a bound is None, ("in", v) or ("ex", v), v in the column's u64 space.  -> (handle, weight):
        a RawHandle for the raw_* helpers' term lists — STAR (= TERM_ALL) where the reference answers with an AllScorer —
        and the weight the clause scores."""
        lk, lv = (0, 0) if lower is None else (BOUND_KINDS[lower[0]], int(lower[1]))
        uk, uv = (0, 0) if upper is None else (BOUND_KINDS[upper[0]], int(upper[1]))
        out, w = C.c_uint32(), C.c_float()
        _check(lib().tq_range_prepare(self.segment_raw(segment_ord), int(column), lk, lv, uk, uv, float(boost), C.byref(out), C.byref(w)))
        return (STAR if out.value == TERM_ALL else RawHandle(out.value)), float(w.value)

    def decode_postings(self, term_id, doc_freq, segment_ord=0):
        h = self.term_handle(term_id, segment_ord)
        if h == TERM_ABSENT:
            raise TantivyAmdError(1, lib().tq_last_error().decode() or "term absent")
        docs = np.zeros(max(1, doc_freq), np.uint32)
        tfs = np.zeros(max(1, doc_freq), np.uint32)
        _check(lib().tq_decode_postings(self.segment_raw(segment_ord), h, _u32(docs), _u32(tfs)))
        return docs[:doc_freq], tfs[:doc_freq]

    def term_table(self, handle, which, segment_ord=0):
        """tq_term_table_read (diagnostic): one derived table of the HANDLE's list, or of the segment (`handle` ignored),
        as the device holds it -> numpy array of the table's element type (TERM_TABLES), empty if the list has no such
        table.  "rec" is (n_blocks + 1, 4), "dense" (words, 2): {doc bits, rank}."""
        w, dtype = TERM_TABLES[which]
        seg, n = self.segment_raw(segment_ord), C.c_uint64()
        _check(lib().tq_term_table_read(seg, int(handle), w, None, 0, C.byref(n)))
        out = np.zeros(int(n.value), np.uint8)
        if n.value:
            _check(lib().tq_term_table_read(seg, int(handle), w, out.ctypes.data, out.size, C.byref(n)))
        out = out[:out.size - out.size % np.dtype(dtype).itemsize].view(dtype)
        return out.reshape(-1, 4) if which == "rec" else (out.reshape(-1, 2) if which in ("dense", "probe_dense") else out)

    def term_table_info(self, handle, segment_ord=0):
        """tq_term_table_info (diagnostic) -> dict of the list's preparation facts (tq_term_table_info_t)."""
        info = TqTermTableInfo()
        _check(lib().tq_term_table_info(self.segment_raw(segment_ord), int(handle), C.byref(info)))
        return {n: int(getattr(info, n)) for n, _ in TqTermTableInfo._fields_}

    def decode_position_deltas(self, term_id, cap, segment_ord=0):
        h = self.term_handle(term_id, segment_ord)
        out = np.zeros(max(1, cap), np.uint32)
        n = C.c_uint64()
        _check(lib().tq_decode_position_deltas(self.segment_raw(segment_ord), h, _u32(out), cap,
                                               C.byref(n)))
        return out[: min(cap, n.value)], n.value

    def set_alive_bitset(self, alive_bytes, segment_ord=0):
        """alive_bytes: the `.del` body (BitSet::serialize) as bytes / np.uint8, or None."""
        if alive_bytes is None:
            _check(lib().tq_segment_set_alive_bitset(self.segment_raw(segment_ord), None, 0))
            return
        a = np.ascontiguousarray(np.frombuffer(bytes(alive_bytes), dtype=np.uint8))
        _check(lib().tq_segment_set_alive_bitset(self.segment_raw(segment_ord), a.ctypes.data,
                                                 a.size))

    def last_batch_match_counts(self, n, segment_ord=0):
        out = np.zeros(max(1, n), np.uint32)
        _check(lib().tq_last_batch_match_counts(self.segment_raw(segment_ord), _u32(out), n))
        return out[:n]

    def last_batch_slop_overflows(self, n, segment_ord=0):
        """Per query of the last batch: candidate docs of a sloppy phrase whose carried position list went over
        SLOP_CARRY_CAP (tq_last_batch_slop_overflows; non-zero = that query's rows are not valid)."""
        out = np.zeros(max(1, n), np.uint32)
        _check(lib().tq_last_batch_slop_overflows(self.segment_raw(segment_ord), _u32(out), n))
        return out[:n]

    def last_batch_query_kernels(self, n, segment_ord=0):
        """TQ_KERNEL_* bit of every query of the last batch (option "record_query_kernels" set before it)."""
        out = np.zeros(max(1, n), np.uint32)
        _check(lib().tq_last_batch_query_kernels(self.segment_raw(segment_ord), _u32(out), n))
        return out[:n]

    def set_option(self, name, value, segment_ord=None):
        ords = range(self.n_segments) if segment_ord is None else [segment_ord]
        for o in ords:
            _check(lib().tq_set_option(self.segment_raw(o), name.encode(), int(value)))

    def last_batch_stats(self, segment_ord=0):
        st = TqBatchStats()
        _check(lib().tq_last_batch_stats(self.segment_raw(segment_ord), C.byref(st)))
        return {"algorithmic_bytes": st.algorithmic_bytes, "matches": st.matches,
                "kernel_ms": st.kernel_ms, "total_ms": st.total_ms, "tiles": st.tiles,
                "chunks": st.chunks, "batches_averaged": st.batches_averaged,
                "host_plan_ms": st.host_plan_ms, "kernel_mask": int(st.kernel_mask),
                "kernels": kernel_names(int(st.kernel_mask)), "unique_bytes": int(st.unique_bytes)}

    def segment_stats(self, segment_ord=0):
        """Resident HBM bytes of one segment by kind (tq_segment_get_stats)."""
        st = TqSegmentStats()
        _check(lib().tq_segment_get_stats(self.segment_raw(segment_ord), C.byref(st)))
        out = {n: int(getattr(st, n)) for n, _ in TqSegmentStats._fields_}
        out["derived_bytes"] = (out["term_table_bytes"] + out["bitmap_bytes"] + out["docmat_bytes"]
                                + out["posdir_bytes"] + out["lead_mat_bytes"])
        out["tantivy_bytes"] = (out["index_bytes"] + out["positions_bytes"] + out["fieldnorm_bytes"]
                                + out["alive_bytes"])
        return out

    def _raw_flat_queries(self, queries, segment_ord):
        """tq_query structs without scoring fields from the tuples _host_queries takes: (mode, [term ids]),
        (MODE_PHRASE, [term ids], [offsets]) or (MODE_BOOL, [term ids], [occurs][, clause_of | None[, min_should_match]])
        with an optional trailing dict {"nested_occurs": [...]}.  -> (array, keep-alive list)"""
        n = len(queries)
        qs = (TqQuery * max(1, n))()
        keep = []
        for i, q in enumerate(queries):
            extra = q[-1] if isinstance(q[-1], dict) else None
            if extra is not None:
                q = q[:-1]
            mode, terms = q[0], q[1]
            hs = (C.c_uint32 * max(1, len(terms)))(*[self.term_handle(t, segment_ord) for t in terms])
            keep.append(hs)
            qs[i].n_terms = len(terms)
            qs[i].terms = C.cast(hs, C.POINTER(C.c_uint32))
            qs[i].mode = mode
            qs[i].k = 1
            if mode == MODE_BOOL:
                oc = (C.c_uint8 * len(terms))(*[int(o) for o in q[2]])
                keep.append(oc)
                qs[i].occurs = C.cast(oc, C.POINTER(C.c_uint8))
                if len(q) > 3 and q[3] is not None:
                    co = (C.c_uint8 * len(terms))(*[int(o) for o in q[3]])
                    keep.append(co)
                    qs[i].clause_of = C.cast(co, C.POINTER(C.c_uint8))
                if len(q) > 4:
                    qs[i].min_should_match = int(q[4])
                if extra and extra.get("nested_occurs") is not None:
                    na = (C.c_uint8 * len(terms))(*[int(o) for o in extra["nested_occurs"]])
                    keep.append(na)
                    qs[i].nested_occurs = C.cast(na, C.POINTER(C.c_uint8))
                # the rest of a tree (doc sets under the option "docset_trees"): conjunctions / phrases, nested minimums
                if extra and extra.get("atom_of") is not None:
                    aa = (C.c_uint8 * len(terms))(*[int(o) for o in extra["atom_of"]])
                    keep.append(aa)
                    qs[i].atom_of = C.cast(aa, C.POINTER(C.c_uint8))
                if extra and extra.get("phrase_offsets") is not None:
                    pa = (C.c_uint32 * len(terms))(*[int(o) for o in extra["phrase_offsets"]])
                    keep.append(pa)
                    qs[i].phrase_offsets = C.cast(pa, C.POINTER(C.c_uint32))
                if extra and extra.get("clause_min_should") is not None:  # {clause_of value: nested minimum}
                    ma = (C.c_uint8 * 16)(*[int(extra["clause_min_should"].get(c, 0)) for c in range(16)])
                    keep.append(ma)
                    qs[i].clause_min_should = C.cast(ma, C.POINTER(C.c_uint8))
            elif mode == MODE_PHRASE:
                oa = (C.c_uint32 * len(terms))(*(q[2] if len(q) > 2 and q[2] is not None else range(len(terms))))
                keep.append(oa)
                qs[i].phrase_offsets = C.cast(oa, C.POINTER(C.c_uint32))
                if len(q) > 3:  # (MODE_PHRASE, [ids], [offsets] | None, slop)
                    qs[i].slop = int(q[3])
        return qs, keep

    def raw_docset(self, queries, cap, segment_ord=0, guard=0, fill=0xDEADBEEF):
        """Direct tq_docset_batch on one segment with a buffer of `cap` docs -> (rc, docs, starts).  docs has cap + guard
        entries preset to `fill` (the call may write the first cap only); starts has len(queries) + 1 entries."""
        n = len(queries)
        qs, keep = self._raw_flat_queries(queries, segment_ord)
        docs = np.full(max(1, cap + guard), fill, np.uint32)
        starts = np.zeros(n + 1, np.uint64)
        rc = lib().tq_docset_batch(self.segment_raw(segment_ord), qs, n, _u32(docs), int(cap),
                                   starts.ctypes.data_as(C.POINTER(C.c_uint64)))
        return rc, docs[: cap + guard], starts

    def raw_docset_device(self, queries, d_docs, cap, d_starts, segment_ord=0, stream=None):
        """Direct tq_docset_batch_device: d_docs (int32 / uint32, at least cap entries) and d_starts (int64 / uint64,
        len(queries) + 1 entries) are torch tensors on the segment's GPU; only enqueues.  -> rc"""
        qs, keep = self._raw_flat_queries(queries, segment_ord)
        return lib().tq_docset_batch_device(self.segment_raw(segment_ord), qs, len(queries), d_docs.data_ptr(), int(cap),
                                            d_starts.data_ptr(), C.c_void_p(stream) if stream else None)

    # ---- sort by fast field (tq_sort.cpp, tq_sort.hip)
    def _raw_sorted_queries(self, queries, ks, segment_ord):
        qs, keep = self._raw_flat_queries(queries, segment_ord)
        ks = [int(ks)] * len(queries) if np.isscalar(ks) else [int(k) for k in ks]
        assert len(ks) == len(queries)
        for i, k in enumerate(ks):
            qs[i].k = k
        return qs, keep, ks

    def raw_search_sorted(self, queries, column, order, nulls, ks, stride=None, segment_ord=0, device=False):
        """Direct tq_search_sorted_batch on one segment: the query tuples of raw_docset, `ks` = one k or one per query,
        stride = the rows' length (default: the largest k).  -> (docs [n, stride] uint32, values [n, stride] uint64,
        has_value [n, stride] uint8, counts [n] uint32).  device=True: through tq_search_sorted_batch_device into torch
        tensors on the segment's GPU, copied back after a synchronisation."""
        n = len(queries)
        qs, keep, ks = self._raw_sorted_queries(queries, ks, segment_ord)
        stride = int(stride) if stride is not None else max(ks + [1])
        if device:
            import torch

            dv = torch.device("cuda", self._devs[segment_ord % len(self._devs)])  # (where __init__ put the segment)
            d_docs = torch.full((max(1, n), stride), 0x5A5A5A5A, dtype=torch.int32, device=dv)
            d_vals = torch.full((max(1, n), stride), 0x5A5A5A5A, dtype=torch.int64, device=dv)
            d_has = torch.full((max(1, n), stride), 0x5A, dtype=torch.uint8, device=dv)
            d_cnt = torch.full((max(1, n),), 0x5A5A5A5A, dtype=torch.int32, device=dv)
            torch.cuda.synchronize(dv)
            _check(lib().tq_search_sorted_batch_device(self.segment_raw(segment_ord), qs, n, int(column), int(order), int(nulls),
                                                       stride, d_docs.data_ptr(), d_vals.data_ptr(), d_has.data_ptr(),
                                                       d_cnt.data_ptr(), None))
            self.last_batch_stats(segment_ord)  # (waits for the segment's stream)
            torch.cuda.synchronize(dv)
            return (d_docs.cpu().numpy().view(np.uint32)[:n], d_vals.cpu().numpy().view(np.uint64)[:n],
                    d_has.cpu().numpy()[:n], d_cnt.cpu().numpy().view(np.uint32)[:n])
        docs = np.full((max(1, n), stride), 0xDEADBEEF, np.uint32)
        vals = np.full((max(1, n), stride), 0xDEADBEEF, np.uint64)
        has = np.full((max(1, n), stride), 0xEF, np.uint8)
        counts = np.full(max(1, n), 0xDEADBEEF, np.uint32)
        _check(lib().tq_search_sorted_batch(self.segment_raw(segment_ord), qs, n, int(column), int(order), int(nulls), stride,
                                            _u32(docs), vals.ctypes.data_as(C.POINTER(C.c_uint64)),
                                            has.ctypes.data_as(C.POINTER(C.c_uint8)), _u32(counts)))
        return docs[:n], vals[:n], has[:n], counts[:n]

    def raw_search_sorted_device(self, queries, column, order, nulls, ks, stride, d_docs, d_values, d_has_value, d_counts,
                                 segment_ord=0, stream=None):
        """Direct tq_search_sorted_batch_device: d_docs (int32 / uint32), d_values (int64 / uint64), d_has_value (uint8) with
        len(queries) * stride entries and d_counts (int32 / uint32, len(queries)) are torch tensors on the segment's GPU;
        only enqueues.  -> rc"""
        qs, keep, ks = self._raw_sorted_queries(queries, ks, segment_ord)
        return lib().tq_search_sorted_batch_device(self.segment_raw(segment_ord), qs, len(queries), int(column), int(order),
                                                   int(nulls), int(stride), d_docs.data_ptr(), d_values.data_ptr(),
                                                   d_has_value.data_ptr(), d_counts.data_ptr(),
                                                   C.c_void_p(stream) if stream else None)

    # ---- aggregations over a fast field (tq_agg.cpp, tq_agg.hip)
    def raw_agg(self, queries, column, value_type, histogram=None, segment_ord=0, device=False, stride=None):
        """Direct tq_agg_batch on one segment: the query tuples of raw_docset; histogram = None (stats alone) or {"interval",
        "offset", "hard_bounds": (min, max)}.  -> (stats: structured array [n] of AGG_STATS_DTYPE, buckets [n, n_buckets]
        uint32, plan dict of agg_histogram_plan — n_buckets 0 without a histogram).  stride: the rows' stride in the call
        (default n_buckets); device=True: through tq_agg_batch_device into torch tensors on the segment's GPU."""
        n = len(queries)
        qs, keep = self._raw_flat_queries(queries, segment_ord)
        req = _agg_request(column, value_type, histogram)
        plan = TqAggHistPlan()
        if histogram is not None:  # (the call makes the same plan; a refusal comes from the call, under its name)
            info = TqColumnInfo()
            if lib().tq_column_info(self.segment_raw(segment_ord), int(column), C.byref(info)) == 0:
                lib().tq_agg_histogram_plan(C.byref(info), C.byref(req), C.byref(plan))
        nb = int(plan.n_buckets)
        stride = nb if stride is None else int(stride)
        stats = np.zeros(max(1, n), AGG_STATS_DTYPE)
        if device:
            import torch

            dv = torch.device("cuda", self._devs[segment_ord % len(self._devs)])  # (where __init__ put the segment)
            d_stats = torch.full((max(1, n), 8), 0x5A5A5A5A, dtype=torch.int64, device=dv)
            d_rows = torch.full((max(1, n), max(1, stride)), 0x5A5A5A5A, dtype=torch.int32, device=dv)
            torch.cuda.synchronize(dv)
            _check(lib().tq_agg_batch_device(self.segment_raw(segment_ord), qs, n, C.byref(req), d_stats.data_ptr(),
                                             d_rows.data_ptr(), stride, None))
            self.last_batch_stats(segment_ord)  # (waits for the segment's stream)
            torch.cuda.synchronize(dv)
            stats = d_stats.cpu().numpy().view(np.uint64).reshape(-1).view(AGG_STATS_DTYPE)
            rows = d_rows.cpu().numpy().view(np.uint32)
        else:
            rows = np.full((max(1, n), max(1, stride)), 0xDEADBEEF, np.uint32)
            _check(lib().tq_agg_batch(self.segment_raw(segment_ord), qs, n, C.byref(req), stats.ctypes.data, _u32(rows), stride))
        return stats[:n], rows[:n, :nb], _agg_plan_dict(plan, req)

    def raw_agg_device(self, queries, column, value_type, histogram, stride, d_stats, d_buckets, segment_ord=0, stream=None):
        """Direct tq_agg_batch_device: d_stats (int64 / uint64, 8 words per query) and d_buckets (int32 / uint32,
        len(queries) * stride entries, or None without a histogram) are torch tensors on the segment's GPU; only enqueues.
        -> rc"""
        qs, keep = self._raw_flat_queries(queries, segment_ord)
        req = _agg_request(column, value_type, histogram)
        return lib().tq_agg_batch_device(self.segment_raw(segment_ord), qs, len(queries), C.byref(req), d_stats.data_ptr(),
                                         d_buckets.data_ptr() if d_buckets is not None else None, int(stride),
                                         C.c_void_p(stream) if stream else None)

    # ---- sub-aggregations (tq_agg.cpp, tq_agg_sub.hip)
    def raw_agg_sub(self, queries, column, value_type, histogram, metric_column, metric_value_type, segment_ord=0, device=False,
                    stride=None):
        """Direct tq_agg_sub_batch on one segment: raw_agg's arguments for the bucket column (histogram = None is refused by
        the call) and the metric column with its value type.  -> (stats, buckets [n, n_buckets] uint32, bucket_stats
        [n, n_buckets] of AGG_BUCKET_STATS_DTYPE, plan dict).  stride: the stride of both kinds of rows in the call (default
        n_buckets); device=True: through tq_agg_sub_batch_device into torch tensors on the segment's GPU."""
        n = len(queries)
        qs, keep = self._raw_flat_queries(queries, segment_ord)
        req = _agg_request(column, value_type, histogram)
        metric = TqAggMetricRequest(column=int(metric_column), value_type=int(metric_value_type))
        plan = TqAggHistPlan()
        if histogram is not None:  # (the call makes the same plan; a refusal comes from the call, under its name)
            info = TqColumnInfo()
            if lib().tq_column_info(self.segment_raw(segment_ord), int(column), C.byref(info)) == 0:
                lib().tq_agg_histogram_plan(C.byref(info), C.byref(req), C.byref(plan))
        nb = int(plan.n_buckets)
        stride = nb if stride is None else int(stride)
        stats = np.zeros(max(1, n), AGG_STATS_DTYPE)
        if device:
            import torch

            dv = torch.device("cuda", self._devs[segment_ord % len(self._devs)])  # (where __init__ put the segment)
            d_stats = torch.full((max(1, n), 8), 0x5A5A5A5A, dtype=torch.int64, device=dv)
            d_rows = torch.full((max(1, n), max(1, stride)), 0x5A5A5A5A, dtype=torch.int32, device=dv)
            d_recs = torch.full((max(1, n), max(1, stride) * 5), 0x5A5A5A5A, dtype=torch.int64, device=dv)
            torch.cuda.synchronize(dv)
            _check(lib().tq_agg_sub_batch_device(self.segment_raw(segment_ord), qs, n, C.byref(req), C.byref(metric),
                                                 d_stats.data_ptr(), d_rows.data_ptr(), d_recs.data_ptr(), stride, None))
            self.last_batch_stats(segment_ord)  # (waits for the segment's stream)
            torch.cuda.synchronize(dv)
            stats = d_stats.cpu().numpy().view(np.uint64).reshape(-1).view(AGG_STATS_DTYPE)
            rows = d_rows.cpu().numpy().view(np.uint32)
            recs = d_recs.cpu().numpy().view(np.uint64).reshape(-1).view(AGG_BUCKET_STATS_DTYPE).reshape(max(1, n), max(1, stride))
        else:
            rows = np.full((max(1, n), max(1, stride)), 0xDEADBEEF, np.uint32)
            recs = np.full((max(1, n), max(1, stride) * 5), 0xDEADBEEF, np.uint64)
            _check(lib().tq_agg_sub_batch(self.segment_raw(segment_ord), qs, n, C.byref(req), C.byref(metric), stats.ctypes.data,
                                          _u32(rows), recs.ctypes.data, stride))
            recs = recs.reshape(-1).view(AGG_BUCKET_STATS_DTYPE).reshape(max(1, n), max(1, stride))
        return stats[:n], rows[:n, :nb], recs[:n, :nb], _agg_plan_dict(plan, req)

    def raw_agg_sub_device(self, queries, column, value_type, histogram, metric_column, metric_value_type, stride, d_stats,
                           d_buckets, d_bucket_stats, segment_ord=0, stream=None):
        """Direct tq_agg_sub_batch_device: raw_agg_device's tensors and d_bucket_stats (int64 / uint64, 5 words per entry,
        len(queries) * stride entries; or None) on the segment's GPU; only enqueues.  -> rc"""
        qs, keep = self._raw_flat_queries(queries, segment_ord)
        req = _agg_request(column, value_type, histogram)
        metric = TqAggMetricRequest(column=int(metric_column), value_type=int(metric_value_type))
        return lib().tq_agg_sub_batch_device(self.segment_raw(segment_ord), qs, len(queries), C.byref(req), C.byref(metric),
                                             d_stats.data_ptr(), d_buckets.data_ptr() if d_buckets is not None else None,
                                             d_bucket_stats.data_ptr() if d_bucket_stats is not None else None, int(stride),
                                             C.c_void_p(stream) if stream else None)

    # ---- range aggregation (tq_agg_range.cpp, tq_agg_range.hip)
    def raw_agg_range(self, queries, column, value_type, ranges, metric_column=None, metric_value_type=None, segment_ord=0,
                      device=False, stride=None):
        """Direct tq_agg_range_batch on one segment: the query tuples of raw_docset; ranges = (from, to) pairs or dicts with
        "from" / "to", None = open; metric_column = None: doc counts alone.  -> (stats: structured array [n] of
        AGG_STATS_DTYPE, counts [n, n_buckets] uint32, bucket_stats [n, n_buckets] of AGG_BUCKET_STATS_DTYPE or None, plan of
        agg_range_plan).  stride: the stride of both kinds of rows in the call (default n_buckets); device=True: through
        tq_agg_range_batch_device into torch tensors on the segment's GPU."""
        n = len(queries)
        qs, keep = self._raw_flat_queries(queries, segment_ord)
        req, keep_ranges = _agg_range_request(column, value_type, ranges)
        with_metric = metric_column is not None
        metric = TqAggMetricRequest(column=int(metric_column), value_type=int(metric_value_type or 0)) if with_metric else None
        mref = C.byref(metric) if with_metric else None
        _, plan = _agg_range_plan(req)  # (the call makes the same plan; a refusal comes from the call, under its name)
        nb = len(plan)
        stride = nb if stride is None else int(stride)
        stats = np.zeros(max(1, n), AGG_STATS_DTYPE)
        if device:
            import torch

            dv = torch.device("cuda", self._devs[segment_ord % len(self._devs)])  # (where __init__ put the segment)
            d_stats = torch.full((max(1, n), 8), 0x5A5A5A5A, dtype=torch.int64, device=dv)
            d_rows = torch.full((max(1, n), max(1, stride)), 0x5A5A5A5A, dtype=torch.int32, device=dv)
            d_recs = torch.full((max(1, n), max(1, stride) * 5), 0x5A5A5A5A, dtype=torch.int64, device=dv)
            torch.cuda.synchronize(dv)
            _check(lib().tq_agg_range_batch_device(self.segment_raw(segment_ord), qs, n, C.byref(req), mref, d_stats.data_ptr(),
                                                   d_rows.data_ptr(), d_recs.data_ptr(), stride, None))
            self.last_batch_stats(segment_ord)  # (waits for the segment's stream)
            torch.cuda.synchronize(dv)
            stats = d_stats.cpu().numpy().view(np.uint64).reshape(-1).view(AGG_STATS_DTYPE)
            rows = d_rows.cpu().numpy().view(np.uint32)
            recs = d_recs.cpu().numpy().view(np.uint64).reshape(-1).view(AGG_BUCKET_STATS_DTYPE).reshape(max(1, n), max(1, stride))
        else:
            rows = np.full((max(1, n), max(1, stride)), 0xDEADBEEF, np.uint32)
            recs = np.full((max(1, n), max(1, stride) * 5), 0xDEADBEEF, np.uint64)
            _check(lib().tq_agg_range_batch(self.segment_raw(segment_ord), qs, n, C.byref(req), mref, stats.ctypes.data,
                                            _u32(rows), recs.ctypes.data, stride))
            recs = recs.reshape(-1).view(AGG_BUCKET_STATS_DTYPE).reshape(max(1, n), max(1, stride))
        return stats[:n], rows[:n, :nb], recs[:n, :nb] if with_metric else None, plan

    def raw_agg_range_device(self, queries, column, value_type, ranges, metric_column, metric_value_type, stride, d_stats, d_counts,
                             d_bucket_stats, segment_ord=0, stream=None):
        """Direct tq_agg_range_batch_device: raw_agg_sub_device's tensors (d_bucket_stats None without a metric) on the
        segment's GPU; only enqueues.  -> rc"""
        qs, keep = self._raw_flat_queries(queries, segment_ord)
        req, keep_ranges = _agg_range_request(column, value_type, ranges)
        metric = None
        if metric_column is not None:
            metric = TqAggMetricRequest(column=int(metric_column), value_type=int(metric_value_type or 0))
        return lib().tq_agg_range_batch_device(self.segment_raw(segment_ord), qs, len(queries), C.byref(req),
                                               C.byref(metric) if metric is not None else None, d_stats.data_ptr(),
                                               d_counts.data_ptr() if d_counts is not None else None,
                                               d_bucket_stats.data_ptr() if d_bucket_stats is not None else None, int(stride),
                                               C.c_void_p(stream) if stream else None)

    # ---- terms aggregation (tq_agg_terms.cpp, tq_agg_terms.hip)
    def agg_terms_plan(self, column, order=TERMS_COUNT_DESC, segment_size=10, segment_ord=0):
        """tq_agg_terms_plan of a resident column: {"n_keys", "min_value", "gcd"}."""
        return agg_terms_plan(self.column_info(column, segment_ord), order, segment_size)

    def raw_agg_terms(self, queries, column, order=TERMS_COUNT_DESC, segment_size=10, segment_ord=0, device=False, stride=None):
        """Direct tq_agg_terms_batch on one segment: the query tuples of raw_docset.  -> (terms: structured array [n] of
        AGG_TERMS_DTYPE, keys [n, width] uint64, counts [n, width] uint32, plan dict of agg_terms_plan), width =
        min(segment_size, n_keys); of row q the first terms[q]["n_returned"] entries are the result, in the request's order.
        stride: the rows' stride in the call (default width); device=True: through tq_agg_terms_batch_device into torch
        tensors on the segment's GPU (entries past n_returned keep the fill)."""
        n = len(queries)
        qs, keep = self._raw_flat_queries(queries, segment_ord)
        req = TqAggTermsRequest(column=int(column), order=int(order), segment_size=int(segment_size))
        plan = TqAggTermsPlan()
        info = TqColumnInfo()  # (the call makes the same plan; a refusal comes from the call, under its name)
        if lib().tq_column_info(self.segment_raw(segment_ord), int(column), C.byref(info)) == 0:
            lib().tq_agg_terms_plan(C.byref(info), C.byref(req), C.byref(plan))
        width = min(int(segment_size), int(plan.n_keys))
        stride = width if stride is None else int(stride)
        if device:
            import torch

            dv = torch.device("cuda", self._devs[segment_ord % len(self._devs)])  # (where __init__ put the segment)
            d_terms = torch.full((max(1, n), 5), 0x5A5A5A5A, dtype=torch.int64, device=dv)
            d_keys = torch.full((max(1, n), max(1, stride)), 0x5A5A5A5A, dtype=torch.int64, device=dv)
            d_counts = torch.full((max(1, n), max(1, stride)), 0x5A5A5A5A, dtype=torch.int32, device=dv)
            torch.cuda.synchronize(dv)
            _check(lib().tq_agg_terms_batch_device(self.segment_raw(segment_ord), qs, n, C.byref(req), d_terms.data_ptr(),
                                                   d_keys.data_ptr(), d_counts.data_ptr(), stride, None))
            self.last_batch_stats(segment_ord)  # (waits for the segment's stream)
            torch.cuda.synchronize(dv)
            terms = d_terms.cpu().numpy().view(np.uint64).reshape(-1).view(AGG_TERMS_DTYPE)
            keys = d_keys.cpu().numpy().view(np.uint64)
            counts = d_counts.cpu().numpy().view(np.uint32)
        else:
            terms = np.zeros(max(1, n), AGG_TERMS_DTYPE)
            keys = np.full((max(1, n), max(1, stride)), 0xDEADBEEF, np.uint64)
            counts = np.full((max(1, n), max(1, stride)), 0xDEADBEEF, np.uint32)
            _check(lib().tq_agg_terms_batch(self.segment_raw(segment_ord), qs, n, C.byref(req), terms.ctypes.data, keys.ctypes.data,
                                            _u32(counts), stride))
        return terms[:n], keys[:n, :width], counts[:n, :width], _agg_terms_plan_dict(plan)

    def raw_agg_terms_device(self, queries, column, order, segment_size, stride, d_terms, d_keys, d_counts, segment_ord=0,
                             stream=None):
        """Direct tq_agg_terms_batch_device: d_terms (int64 / uint64, 5 words per query), d_keys (int64 / uint64) and d_counts
        (int32 / uint32), len(queries) * stride entries each (or None), are torch tensors on the segment's GPU; only
        enqueues.  -> rc"""
        qs, keep = self._raw_flat_queries(queries, segment_ord)
        req = TqAggTermsRequest(column=int(column), order=int(order), segment_size=int(segment_size))
        return lib().tq_agg_terms_batch_device(self.segment_raw(segment_ord), qs, len(queries), C.byref(req),
                                               d_terms.data_ptr() if d_terms is not None else None,
                                               d_keys.data_ptr() if d_keys is not None else None,
                                               d_counts.data_ptr() if d_counts is not None else None, int(stride),
                                               C.c_void_p(stream) if stream else None)

    # ---- terms aggregation with a metric (tq_agg_terms_sub.cpp, tq_agg_terms_sub.hip)
    def raw_agg_terms_sub(self, queries, column, metric_column, metric_value_type, order=TERMS_COUNT_DESC, segment_size=10,
                          order_metric=METRIC_AVG, segment_ord=0, device=False, stride=None, reserved=(0, 0)):
        """Direct tq_agg_terms_sub_batch on one segment: raw_agg_terms' arguments and the metric column.  -> (terms, keys
        [n, width] uint64, counts [n, width] uint32, records [n, width] of AGG_BUCKET_STATS_DTYPE, plan dict), width =
        min(segment_size, n_keys); of row q the first terms[q]["n_returned"] entries are the result, in the request's order.
        stride: the rows' stride in the call (default width; the rows come back `stride` wide when it is given);
        device=True: through tq_agg_terms_sub_batch_device into torch tensors on the segment's GPU (entries past n_returned
        keep the fill)."""
        n = len(queries)
        qs, keep = self._raw_flat_queries(queries, segment_ord)
        req = TqAggTermsSubRequest(column=int(column), order=int(order), segment_size=int(segment_size), metric_column=int(metric_column),
                                   metric_value_type=int(metric_value_type), order_metric=int(order_metric))
        req.reserved[0], req.reserved[1] = int(reserved[0]), int(reserved[1])
        plan = TqAggTermsPlan()
        info = TqColumnInfo()  # (the call makes the same plan; a refusal comes from the call, under its name)
        if lib().tq_column_info(self.segment_raw(segment_ord), int(column), C.byref(info)) == 0:
            treq = TqAggTermsRequest(column=int(column), order=min(int(order), TERMS_KEY_DESC), segment_size=int(segment_size))
            lib().tq_agg_terms_plan(C.byref(info), C.byref(treq), C.byref(plan))
        width = min(int(segment_size), int(plan.n_keys))
        out_w = width if stride is None else int(stride)
        stride = out_w
        if device:
            import torch

            dv = torch.device("cuda", self._devs[segment_ord % len(self._devs)])  # (where __init__ put the segment)
            d_terms = torch.full((max(1, n), 5), 0x5A5A5A5A, dtype=torch.int64, device=dv)
            d_keys = torch.full((max(1, n), max(1, stride)), 0x5A5A5A5A, dtype=torch.int64, device=dv)
            d_counts = torch.full((max(1, n), max(1, stride)), 0x5A5A5A5A, dtype=torch.int32, device=dv)
            d_recs = torch.full((max(1, n), max(1, stride) * 5), 0x5A5A5A5A, dtype=torch.int64, device=dv)
            torch.cuda.synchronize(dv)
            _check(lib().tq_agg_terms_sub_batch_device(self.segment_raw(segment_ord), qs, n, C.byref(req), d_terms.data_ptr(),
                                                       d_keys.data_ptr(), d_counts.data_ptr(), d_recs.data_ptr(), stride, None))
            self.last_batch_stats(segment_ord)  # (waits for the segment's stream)
            torch.cuda.synchronize(dv)
            terms = d_terms.cpu().numpy().view(np.uint64).reshape(-1).view(AGG_TERMS_DTYPE)
            keys = d_keys.cpu().numpy().view(np.uint64)
            counts = d_counts.cpu().numpy().view(np.uint32)
            recs = d_recs.cpu().numpy().view(np.uint64).reshape(-1).view(AGG_BUCKET_STATS_DTYPE).reshape(max(1, n), max(1, stride))
        else:
            terms = np.zeros(max(1, n), AGG_TERMS_DTYPE)
            keys = np.full((max(1, n), max(1, stride)), 0xDEADBEEF, np.uint64)
            counts = np.full((max(1, n), max(1, stride)), 0xDEADBEEF, np.uint32)
            recs = np.full((max(1, n), max(1, stride) * 5), 0xDEADBEEF, np.uint64).reshape(-1).view(AGG_BUCKET_STATS_DTYPE)
            recs = recs.reshape(max(1, n), max(1, stride))
            _check(lib().tq_agg_terms_sub_batch(self.segment_raw(segment_ord), qs, n, C.byref(req), terms.ctypes.data, keys.ctypes.data,
                                                _u32(counts), recs.ctypes.data, stride))
        return terms[:n], keys[:n, :out_w], counts[:n, :out_w], recs[:n, :out_w], _agg_terms_plan_dict(plan)

    def raw_agg_terms_sub_device(self, queries, column, metric_column, metric_value_type, order, segment_size, order_metric, stride,
                                 d_terms, d_keys, d_counts, d_records, segment_ord=0, stream=None, reserved=(0, 0)):
        """Direct tq_agg_terms_sub_batch_device: raw_agg_terms_device's tensors and d_records (int64 / uint64, 5 words per
        entry, len(queries) * stride entries, or None), torch tensors on the segment's GPU; only enqueues.  -> rc"""
        qs, keep = self._raw_flat_queries(queries, segment_ord)
        req = TqAggTermsSubRequest(column=int(column), order=int(order), segment_size=int(segment_size), metric_column=int(metric_column),
                                   metric_value_type=int(metric_value_type), order_metric=int(order_metric))
        req.reserved[0], req.reserved[1] = int(reserved[0]), int(reserved[1])
        return lib().tq_agg_terms_sub_batch_device(self.segment_raw(segment_ord), qs, len(queries), C.byref(req),
                                                   d_terms.data_ptr() if d_terms is not None else None,
                                                   d_keys.data_ptr() if d_keys is not None else None,
                                                   d_counts.data_ptr() if d_counts is not None else None,
                                                   d_records.data_ptr() if d_records is not None else None, int(stride),
                                                   C.c_void_p(stream) if stream else None)

    # ---- terms x histogram (tq_agg_terms_hist.cpp, tq_agg_terms_hist.hip)
    def agg_terms_hist_plan(self, column, hist_column, value_type, histogram, order=TERMS_COUNT_DESC, segment_size=10, segment_ord=0):
        """tq_agg_terms_hist_plan of two resident columns: {"terms", "hist", "n_cells"}."""
        return agg_terms_hist_plan(self.column_info(column, segment_ord), self.column_info(hist_column, segment_ord), value_type,
                                   histogram, order, segment_size)

    def raw_agg_terms_hist(self, queries, column, hist_column, value_type, histogram, order=TERMS_COUNT_DESC, segment_size=10,
                           segment_ord=0, device=False, stride=None, hist_stride=None, reserved=(0, 0), histogram_flag=1):
        """Direct tq_agg_terms_hist_batch on one segment: raw_agg_terms' arguments, the histogram column with its value type
        and raw_agg's histogram dict.  -> (terms, keys [n, width] uint64, counts [n, width] uint32, rows [n, width, n_buckets]
        uint32, plan dict of agg_terms_hist_plan), width = min(segment_size, n_keys); of row set q the first
        terms[q]["n_returned"] entries are the result, in the request's order.  stride / hist_stride: the strides in the call
        (default width / n_buckets; the arrays come back that wide when given); device=True: through
        tq_agg_terms_hist_batch_device into torch tensors on the segment's GPU (what the call leaves alone keeps the fill)."""
        n = len(queries)
        qs, keep = self._raw_flat_queries(queries, segment_ord)
        req = _agg_terms_hist_request(column, hist_column, value_type, histogram, order, segment_size, reserved, histogram_flag)
        plan = TqAggTermsHistPlan()
        it, ih = TqColumnInfo(), TqColumnInfo()  # (the call makes the same plan; a refusal comes from the call, under its name)
        seg = self.segment_raw(segment_ord)
        if lib().tq_column_info(seg, int(column), C.byref(it)) == 0 and lib().tq_column_info(seg, int(hist_column), C.byref(ih)) == 0:
            lib().tq_agg_terms_hist_plan(C.byref(it), C.byref(ih), C.byref(req), C.byref(plan))
        width, n_buckets = min(int(segment_size), int(plan.terms.n_keys)), int(plan.hist.n_buckets)
        out_w = width if stride is None else int(stride)
        out_b = n_buckets if hist_stride is None else int(hist_stride)
        shape = (max(1, n), max(1, out_w))
        if device:
            import torch

            dv = torch.device("cuda", self._devs[segment_ord % len(self._devs)])  # (where __init__ put the segment)
            d_terms = torch.full((max(1, n), 5), 0x5A5A5A5A, dtype=torch.int64, device=dv)
            d_keys = torch.full(shape, 0x5A5A5A5A, dtype=torch.int64, device=dv)
            d_counts = torch.full(shape, 0x5A5A5A5A, dtype=torch.int32, device=dv)
            d_rows = torch.full(shape + (max(1, out_b),), 0x5A5A5A5A, dtype=torch.int32, device=dv)
            torch.cuda.synchronize(dv)
            _check(lib().tq_agg_terms_hist_batch_device(seg, qs, n, C.byref(req), d_terms.data_ptr(), d_keys.data_ptr(),
                                                        d_counts.data_ptr(), d_rows.data_ptr(), out_w, out_b, None))
            self.last_batch_stats(segment_ord)  # (waits for the segment's stream)
            torch.cuda.synchronize(dv)
            terms = d_terms.cpu().numpy().view(np.uint64).reshape(-1).view(AGG_TERMS_DTYPE)
            keys = d_keys.cpu().numpy().view(np.uint64)
            counts = d_counts.cpu().numpy().view(np.uint32)
            rows = d_rows.cpu().numpy().view(np.uint32)
        else:
            terms = np.zeros(max(1, n), AGG_TERMS_DTYPE)
            keys = np.full(shape, 0xDEADBEEF, np.uint64)
            counts = np.full(shape, 0xDEADBEEF, np.uint32)
            rows = np.full(shape + (max(1, out_b),), 0xDEADBEEF, np.uint32)
            _check(lib().tq_agg_terms_hist_batch(seg, qs, n, C.byref(req), terms.ctypes.data, keys.ctypes.data, _u32(counts), _u32(rows),
                                                 out_w, out_b))
        return terms[:n], keys[:n, :out_w], counts[:n, :out_w], rows[:n, :out_w, :out_b], _agg_terms_hist_plan_dict(plan, req)

    def raw_agg_terms_hist_device(self, queries, column, hist_column, value_type, histogram, order, segment_size, stride, hist_stride,
                                  d_terms, d_keys, d_counts, d_rows, segment_ord=0, stream=None, reserved=(0, 0), histogram_flag=1):
        """Direct tq_agg_terms_hist_batch_device: raw_agg_terms_device's tensors and d_rows (int32 / uint32, len(queries) *
        stride * hist_stride entries, or None), torch tensors on the segment's GPU; only enqueues.  -> rc"""
        qs, keep = self._raw_flat_queries(queries, segment_ord)
        req = _agg_terms_hist_request(column, hist_column, value_type, histogram, order, segment_size, reserved, histogram_flag)
        return lib().tq_agg_terms_hist_batch_device(self.segment_raw(segment_ord), qs, len(queries), C.byref(req),
                                                    d_terms.data_ptr() if d_terms is not None else None,
                                                    d_keys.data_ptr() if d_keys is not None else None,
                                                    d_counts.data_ptr() if d_counts is not None else None,
                                                    d_rows.data_ptr() if d_rows is not None else None, int(stride), int(hist_stride),
                                                    C.c_void_p(stream) if stream else None)

    def _raw_scored_queries(self, queries, weights, cache, segment_ord):
        """_raw_flat_queries with the scoring fields: weights = per-query lists of floats (or None: left NULL), cache =
        np.float32[256] (a multi-field segment: np.float32[F, 256], row f = field f's cache; or None), or a list of one per query (the same object = the same pointer; None: left NULL).
        -> (array, keep-alive list)"""
        qs, keep = self._raw_flat_queries(queries, segment_ord)
        per_query = None
        if isinstance(cache, (list, tuple)):
            held = {}
            per_query = [None if c is None else held.setdefault(id(c), np.ascontiguousarray(c, np.float32)) for c in cache]
            keep += list(held.values())
        elif cache is not None:
            cache = np.ascontiguousarray(cache, np.float32)
            keep.append(cache)
        for i in range(len(queries)):
            if weights is not None and weights[i] is not None:
                ws = (C.c_float * max(1, len(weights[i])))(*weights[i])
                keep.append(ws)
                qs[i].weights = C.cast(ws, C.POINTER(C.c_float))
            if per_query is not None:
                if per_query[i] is not None:
                    qs[i].tf_cache = _f32(per_query[i])
            elif cache is not None:
                qs[i].tf_cache = _f32(cache)
        return qs, keep

    def raw_docset_scored(self, queries, cap, segment_ord=0, guard=0, weights=None, cache=None):
        """Direct tq_docset_scored_batch on one segment with buffers of `cap` entries -> (rc, docs, scores, starts).  docs
        and scores have cap + guard entries preset to 0xDEADBEEF (the scores: that bit pattern as f32); weights / cache
        as raw_search takes them (None: the queries' weights / tf_cache stay NULL)."""
        n = len(queries)
        qs, keep = self._raw_scored_queries(queries, weights, cache, segment_ord)
        docs = np.full(max(1, cap + guard), 0xDEADBEEF, np.uint32)
        scores = np.full(max(1, cap + guard), 0xDEADBEEF, np.uint32).view(np.float32)
        starts = np.zeros(n + 1, np.uint64)
        rc = lib().tq_docset_scored_batch(self.segment_raw(segment_ord), qs, n, _u32(docs), _f32(scores), int(cap),
                                          starts.ctypes.data_as(C.POINTER(C.c_uint64)))
        return rc, docs[: cap + guard], scores[: cap + guard], starts

    def raw_docset_scored_device(self, queries, d_docs, d_scores, cap, d_starts, segment_ord=0, stream=None, weights=None,
                                 cache=None):
        """Direct tq_docset_scored_batch_device: d_docs (int32 / uint32), d_scores (float32) with at least cap entries and
        d_starts (int64 / uint64, len(queries) + 1 entries) are torch tensors on the segment's GPU; only enqueues.  -> rc"""
        qs, keep = self._raw_scored_queries(queries, weights, cache, segment_ord)
        return lib().tq_docset_scored_batch_device(self.segment_raw(segment_ord), qs, len(queries), d_docs.data_ptr(),
                                                   d_scores.data_ptr(), int(cap), d_starts.data_ptr(),
                                                   C.c_void_p(stream) if stream else None)

    def raw_search_trees(self, queries, weights, cache, k, opts=None, segment_ord=0, return_rc=False):
        """Direct tq_search_batch_opts over the structs raw_docset_scored sends (_raw_scored_queries: atom_of /
        phrase_offsets / clause_min_should included), every query with top-k size k; weights / cache as
        raw_docset_scored takes them; opts = (exhaustive, bound_slack_ppm) or None
        -> (scores[n, k], docs[n, k], counts[n]); return_rc: (rc, scores, docs, counts) without raising — a sloppy
        phrase over the carry cap is TQ_ERR_UNSUPPORTED with the other queries' rows written."""
        n = len(queries)
        qs, keep = self._raw_scored_queries(queries, weights, cache, segment_ord)
        for i in range(n):
            qs[i].k = int(k)
        scores = np.zeros((max(1, n), k), np.float32)
        docs = np.zeros((max(1, n), k), np.uint32)
        counts = np.zeros(max(1, n), np.uint32)
        o = TqSearchOpts(int(opts[0]), int(opts[1])) if opts is not None else None
        rc = lib().tq_search_batch_opts(self.segment_raw(segment_ord), qs, n, k, _f32(scores), _u32(docs), _u32(counts),
                                        C.byref(o) if o is not None else None)
        if return_rc:
            return rc, scores[:n], docs[:n], counts[:n]
        _check(rc)
        return scores[:n], docs[:n], counts[:n]

    def raw_count(self, queries, weights, cache, segment_ord=0):
        """Direct tq_count_batch (Count collector): alive matches per query."""
        n = len(queries)
        qs = (TqQuery * max(1, n))()
        keep = []
        cache = np.ascontiguousarray(cache, np.float32)
        for i, q in enumerate(queries):
            mode, terms = q[0], q[1]
            hs = (C.c_uint32 * len(terms))(*[self.term_handle(t, segment_ord) for t in terms])
            ws = (C.c_float * len(weights[i]))(*weights[i])
            keep += [hs, ws]
            qs[i].n_terms = len(terms)
            qs[i].terms = C.cast(hs, C.POINTER(C.c_uint32))
            qs[i].weights = C.cast(ws, C.POINTER(C.c_float))
            qs[i].tf_cache = _f32(cache)
            qs[i].mode = mode
            if mode == MODE_PHRASE:
                oa = (C.c_uint32 * len(terms))(*(q[2] if len(q) > 2 and q[2] is not None
                                                 else range(len(terms))))
                keep.append(oa)
                qs[i].phrase_offsets = C.cast(oa, C.POINTER(C.c_uint32))
            if mode == MODE_PHRASE:  # (MODE_PHRASE, [ids], [offsets] | None, slop)
                qs[i].slop = int(q[3]) if len(q) > 3 else 0
            elif len(q) > 3 and q[3] is not None:  # TQ_MODE_BOOL, as raw_search takes it: occurs, clause_of, minimum
                oc = (C.c_uint8 * len(terms))(*q[3])
                keep.append(oc)
                qs[i].occurs = C.cast(oc, C.POINTER(C.c_uint8))
            if len(q) > 4 and q[4] is not None:
                co = (C.c_uint8 * len(terms))(*q[4])
                keep.append(co)
                qs[i].clause_of = C.cast(co, C.POINTER(C.c_uint8))
            if len(q) > 5:
                qs[i].min_should_match = int(q[5])
            qs[i].k = 1
        counts = np.zeros(max(1, n), np.uint32)
        _check(lib().tq_count_batch(self.segment_raw(segment_ord), qs, n, _u32(counts)))
        return counts[:n]

    def raw_search_one(self, query, weights, cache, k, segment_ord=0):
        """Direct tq_search_one (tq_submit + tq_wait) of one query in the tuple form of _raw_flat_queries ->
        (scores[k], docs[k], count)."""
        qs, keep = self._raw_scored_queries([query], [weights], cache, segment_ord)
        qs[0].k = int(k)
        scores = np.zeros(k, np.float32)
        docs = np.zeros(k, np.uint32)
        count = C.c_uint32()
        _check(lib().tq_search_one(self.segment_raw(segment_ord), qs, None, _f32(scores), _u32(docs), C.byref(count)))
        return scores, docs, int(count.value)

    def raw_search(self, queries, weights, cache, k, segment_ord=0, stride=None, opts=None):
        """Direct tq_search_batch[_opts]: queries = list of (mode, [term ids], offsets|None);
        weights = list of per-query float lists; cache = np.float32[256]; opts = (exhaustive,
        bound_slack_ppm) for this call only (tq_search_opts) or None."""
        n = len(queries)
        stride = k if stride is None else stride
        qs = (TqQuery * max(1, n))()
        keep = []
        cache = np.ascontiguousarray(cache, np.float32)
        for i, q in enumerate(queries):
            mode, terms = q[0], q[1]
            hs = (C.c_uint32 * len(terms))(*[self.term_handle(t, segment_ord) for t in terms])
            ws = (C.c_float * len(weights[i]))(*weights[i])
            keep += [hs, ws]
            qs[i].n_terms = len(terms)
            qs[i].terms = C.cast(hs, C.POINTER(C.c_uint32))
            qs[i].weights = C.cast(ws, C.POINTER(C.c_float))
            qs[i].tf_cache = _f32(cache)
            qs[i].mode = mode
            if len(q) > 2 and q[2] is not None:
                oa = (C.c_uint32 * len(terms))(*q[2])
                keep.append(oa)
                qs[i].phrase_offsets = C.cast(oa, C.POINTER(C.c_uint32))
            if mode == MODE_PHRASE:  # (MODE_PHRASE, [ids], [offsets] | None, slop)
                qs[i].slop = int(q[3]) if len(q) > 3 else 0
            elif len(q) > 3 and q[3] is not None:  # TQ_MODE_BOOL: enum tq_occur
                oc = (C.c_uint8 * len(terms))(*q[3])
                keep.append(oc)
                qs[i].occurs = C.cast(oc, C.POINTER(C.c_uint8))
            if len(q) > 4 and q[4] is not None:
                co = (C.c_uint8 * len(terms))(*q[4])
                keep.append(co)
                qs[i].clause_of = C.cast(co, C.POINTER(C.c_uint8))
            if len(q) > 5:
                qs[i].min_should_match = int(q[5])
            qs[i].k = k
        scores = np.zeros((n, stride), np.float32)
        docs = np.zeros((n, stride), np.uint32)
        counts = np.zeros(n, np.uint32)
        if opts is not None:
            o = TqSearchOpts(int(opts[0]), int(opts[1]))
            _check(lib().tq_search_batch_opts(self.segment_raw(segment_ord), qs, n, stride,
                                              _f32(scores), _u32(docs), _u32(counts), C.byref(o)))
        else:
            _check(lib().tq_search_batch(self.segment_raw(segment_ord), qs, n, stride, _f32(scores),
                                         _u32(docs), _u32(counts)))
        return scores, docs, counts
