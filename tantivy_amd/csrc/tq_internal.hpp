// tq_internal.hpp — declarations shared by the translation units of the C ABI library
// (include/tantivy_amd.h): the segment and context objects, device buffers, the host planner's
// scratch and its launch groups, the planner thread pool, and the internal entry points of
//   tq_api.cpp          the ABI's object lifecycle, options, statistics, codec access, merges
//   tq_terms.cpp        tq_term_prepare / tq_term_prepare_batch and its stages, the device walk, term-table sync
//   tq_term_walk.cpp    the host format walker (no HIP call: tools/planbench/walk_check.cpp), the term blob's layout
//   tq_term_arena.cpp   term slabs, the arena of the side tables (hipMalloc or a mapped address range), directory chunks
//   tq_term_tables.cpp  side tables of a list: tf bytes, range maxima, plain arrays, leader norms, doc matrix and
//                       signatures, range directories, the dense lists' bitmaps
//   tq_term_probe.cpp   the probe pool (slots, eviction) and the tables built into it
//   tq_plan_chunks.cpp  tiles -> chunks -> launch order of the per-query kernels
//   tq_plan_share.cpp   the term-major launches: shared unions (leads / tasks), shared intersections
//   tq_plan_misc.cpp    the doc-major union plan, boolean query layout
//   tq_search.cpp       one batch: validate, plan, stage, launch (tq_search_batch*)
//   tq_submit.cpp       tq_submit / tq_wait / tq_search_one: coalescing of concurrent single queries
// Everything here is internal: nothing outside tantivy_amd/csrc (and tools/planbench, which tests the
// planner without a GPU) includes it.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <map>
#include <mutex>
#include <new>
#include <cstdlib>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <thread>
#include <vector>

#include "../../include/tantivy_amd.h"
#include "tq_device.h"
#include "tq_launch.h"
#include "tq_prepare.h"

namespace tqi {

extern thread_local std::string g_last_error;
int fail(int code, const char *fmt, ...);
inline int launched(hipError_t e, const char *what) {  // the verdict on a kernel launch: TQ_OK, or TQ_ERR_HIP naming it
  return e == hipSuccess ? TQ_OK : fail(TQ_ERR_HIP, "%s launch: %s", what, hipGetErrorString(e));
}
#define HIP_TRY(expr)                                                                    \
  do {                                                                                   \
    hipError_t e__ = (expr);                                                             \
    if (e__ != hipSuccess)                                                               \
      return fail(TQ_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__),    \
                  __FILE__, __LINE__);                                                   \
  } while (0)

constexpr size_t PAD = 1088;  // over-read slack after every device byte buffer (staged block loads)

// A grow-only device buffer.
struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;
  // (the old buffer goes first — a grown buffer next to its predecessor would double the peak — and the
  // capacity with it: a failed allocation leaves {null, 0}, never a stale capacity over a null pointer)
  int ensure(size_t n) {
    if (n <= cap) return TQ_OK;
    const size_t ncap = std::max(n, cap * 2);
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    void *np = nullptr;
    HIP_TRY(hipMalloc(&np, ncap));
    p = np;
    cap = ncap;
    return TQ_OK;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};
struct PinnedBuf {
  void *p = nullptr;
  size_t cap = 0;
  int ensure(size_t n) {
    if (n <= cap) return TQ_OK;
    const size_t ncap = std::max(n, cap * 2);
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
    void *np = nullptr;
    HIP_TRY(hipHostMalloc(&np, ncap, hipHostMallocDefault));
    p = np;
    cap = ncap;
    return TQ_OK;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
  }
};

struct TermHost {
  void *blob = nullptr;  // one device allocation holding every per-term array
  const TqdTerm *d_self = nullptr;  // ... and a copy of the term's record as of its upload (rec / coarse / tail /
                                    // payload fields: what the kernels that build its side tables read)
  void *dense_blob = nullptr;  // bitmap + rank directory of a dense list
  void *posdir_blob = nullptr; // position directory of a dense list with positions
  void *tf8_blob = nullptr;    // term freqs of a dense list as bytes (posting index -> min(tf, 255))
  void *pos_blob = nullptr;    // device-side prepare: positions tables (sized after the walk)
  void *probe_dense_blob = nullptr, *probe_tf8_blob = nullptr;  // a list below "dense_ratio" that boolean queries
                               // probe in the shared launch: bitmap + rank directory and tf bytes built on first
                               // use ("probe_budget_x"); the other kernels do not see them
  void *probe_posdir_blob = nullptr;  // ... and its position directory (TqdTerm::pos_dir layout), built the first time
                                      // a phrase INSIDE a boolean query names the list (tq_tree.hip)
  int32_t probe_slot = -1;            // the slot of the segment's probe pool that holds them (tq_term_probe.cpp), or -1
  // a list below "dense_ratio": its range directory (rdir_lookup, tq_common.hpp: one u32 per posting in posting order +
  // a directory of posting counts per 2^rdir_shift docs; 6-8 bytes per posting), built when the term is prepared, while
  // such tables stay within "rdir_budget_x": the shared intersection launch asks it "is d in the list, with which tf" —
  // what a max_doc / 4-byte bitmap + rank directory + tf bytes from the probe pool answered before
  void *rdir_blob = nullptr;          // the directory (256-byte aligned: the shift rides in the low bits of its offset)
  void *rdir_ent = nullptr;           // the entries, right behind it
  uint32_t rdir_shift = 0;
  uint8_t *probe_own_dir = nullptr;   // a list too long for a slot: room for its position directory next to its own tables
  void *rmax_blob = nullptr;   // range maxima of a list with a bitmap (its own or the probe tables'): one byte per
                               // TQD_RM_SHIFT docs, tq_ashare.hip's bound on non-leader lists
  uint32_t rmax_list = 255;    // ... the largest of them
  void *flat_blob = nullptr;   // a list without a bitmap as plain arrays (doc ids | byte-wide tfs), built on
                               // first use by an unpruned union batch (tq_xunion.hip)
  void *lnorm_blob = nullptr;  // the fieldnorm ids of the list's docs in posting order (byte i = fieldnorm[doc of
                               // posting i], 128 bytes per block), built the first time the list LEADS queries of a
                               // shared-intersection launch: stage A reads one line per block instead of 128 gathers
  void *lmat_blob = nullptr;   // the doc-matrix words of the list's docs in posting order (word i = docmat[doc of posting
                               // i], 1 KB per block, zero padding behind the last posting), built like lnorm_blob for a
                               // leader under the "lead_mat_cut": stage A reads one 16-byte load per lane instead of two gathers
  uint64_t lmat_epoch = 0;     // tq_segment::docmat_epoch the table was filled at: it is used only while the two are equal
  uint32_t doc_freq = 0, n_blocks = 0, n_full = 0, n_tail = 0;
  uint32_t last_doc = 0;
  bool wants_col = true;  // false: the segment's columns are reserved for other lists
  uint64_t postings_len = 0, positions_len = 0;
  uint64_t n_positions = 0;
  // a TERM SET (tq_termset.cpp): the slot holds no posting list — dense_blob is the OR of its members' docs, doc_freq the
  // number of docs in it (the reference's cost of a BitSetDocSet), postings_len the bytes of its bits, and it scores
  // its weight as given.  kSetReleased: the tombstone tq_term_set_release leaves (a later set may take the slot)
  enum : uint8_t { kNoSet = 0, kSet = 1, kSetReleased = 2 };
  uint8_t set_kind = kNoSet;
  uint8_t field = 0;  // the field of a multi-field segment the list belongs to (tq_term_prepare_field); 0: the primary field
};

inline uint32_t rd32(const uint8_t *p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
// common VInt (common/src/vint.rs:61-112): stop bit on the LAST byte
inline bool read_vint(const uint8_t *d, size_t len, size_t &at, uint64_t &out) {
  uint64_t r = 0;
  unsigned shift = 0;
  while (at < len) {
    uint8_t b = d[at++];
    r |= (uint64_t)(b & 127u) << shift;
    if (b & 128u) {
      out = r;
      return true;
    }
    shift += 7;
    if (shift > 63) return false;
  }
  return false;
}
inline bool read_vint32_block(const uint8_t *d, size_t len, size_t &at, uint32_t &out) {
  uint32_t r = 0, shift = 0;
  while (at < len) {
    uint8_t b = d[at++];
    r += (uint32_t)(b & 127u) << shift;
    if (b & 128u) {
      out = r;
      return true;
    }
    shift += 7;
  }
  return false;
}

struct Options {
  int exhaustive = 0;  // 0 = block-max pruned top-k (what the reference executes), 1 = score every match
  int timing = 0;
  int use_dpp = 1;
  int dense = 1;      // build bitmaps for dense lists at tq_term_prepare
  int dense_ratio = TQD_DENSE_RATIO;  // ... for lists with doc_freq >= max_doc / dense_ratio
  int dense_budget_x = 8;  // ... while bitmaps + byte-wide tfs + doc matrix + signatures + position directories
                           // stay below this multiple of the segment's bytes
  int use_dense = 1;  // let the scan kernels use them
  int docmat = 1;     // also build the doc-major matrix of the dense lists
  int docsig = 1;     // ... and the per-doc signature word of the lists without a column
  int device_prepare = 0;  // walk skip lists / build dense tables on the device even with a host copy
  int or_windows = -1;  // OR: 1 = window-parallel kernel, 0 = candidate-driven kernel, -1 = auto
  int bound_slack_ppm = 0;  // block-max bounds are widened by (1 + ppm * 1e-6), see block_max_score
                        // (windows for exhaustive scans, candidates when pruning)
  // unpruned unions, doc-major (tq_xunion.hip): queries whose lists together hold at least
  // max_doc / xunion_ratio postings (0 = never), if the batch has at least xunion_min_queries of them
  int xunion_ratio = 64;
  int xunion_min_queries = 64;
  int lead_mat_budget_x = 4;  // leaders' doc-matrix words in posting order (TermHost::lmat_blob, 8 B per posting): at most this
                              // multiple of the segment, 0 = none are built or used
  int lead_mat_cut = 16;      // ... only for leaders whose postings are on average at least this many docs apart (a denser
                              // list's docs share doc-matrix lines: it keeps the gather)
  int rdir_budget_x = 4;    // range directories of the lists below "dense_ratio" (6-8 B per posting): at most this multiple of the segment
  int probe_budget_x = 16;  // bitmaps + tf bytes built on demand for the lists boolean queries probe: at most this multiple of the segment
  int count_bitmap_ratio = 128;  // Count: bitmap words instead of a scan if the driving clause holds >= max_doc / ratio postings per list
  int docset_temp_lists = 0;     // doc sets: lists without a bitmap scattered per launch (0 = what TQ_COUNT_TEMP_MB holds, at most 4096)
  int docset_trees = 0;          // doc sets: phrases and nested boolean queries through tq_docset_tree.hip (0 = refused, as before)
  int docset_score_trees = 0;    // scored doc sets: the same shapes, scored by tq_docset_tree_score.hip (0 = refused, as before)
  int sort_slices = 0;           // sort by fast field: slices of the bitmap words per query (0 = the host chooses, 1..256 = forced)
  int agg_slices = 0;            // aggregations: the same for tq_agg_batch*
  int agg_lds_buckets = -1;      // aggregations: the largest histogram that goes through LDS (-1 = the kernel's capacity)
  int ashare_inline_warm = 1;   // intersections: 0 = warm-up and main tasks as two dispatches, 1 = ONE dispatch where they are the batch's only
                                // group and tasks of leaders without warm-up tasks fill the grid (build_ashare_plan), 2 = always one dispatch
  int ashare_min_batch = 16;    // intersections: the shared launch needs this many qualifying queries in the batch (512 until round 6)
  // tq_submit / tq_search_one: how long the leader of a batch waits for the callers of the previous
  // batch to come back with their next query (0 = launch with whatever is pending)
  int submit_window_us = 100;
  int record_query_kernels = 0;  // tq_last_batch_query_kernels: remember which scan-kernel family ran every query
  int debug = -1;  // >= 0: overrides TQ_DEBUG for this segment's launches (work counters / ablations: diagnosis only)
};


inline uint32_t tune_u32(const char *name, uint32_t dflt) {
  const char *v = getenv(name);
  return v && *v ? (uint32_t)strtoul(v, nullptr, 10) : dflt;
}

}  // namespace tqi
using namespace tqi;  // (the objects below are the ABI's opaque types: global)

// The big per-batch buffers — partial / result lists, the staging lists of the two term-major launches —
// exist once per DEVICE, not once per segment: a device runs one batch at a time anyway (the kernels fill
// it), and 100 segments on a GPU must not mean 100 copies (8 segments held 13.9 GB of scratch in round 3).
// A batch takes the lock when it sizes the buffers and keeps it until the event behind its last kernel is
// recorded; a batch on another stream than the previous user's first waits for that event (stream side).
struct DeviceScratch {
  std::mutex m;
  DevBuf partials, share_stage, ashare_stage, bshare_stage;
  hipEvent_t ev_last = nullptr;
  hipStream_t last_stream = nullptr;
  bool in_flight = false;
};
struct tq_ctx {
  std::vector<int> devices;
  std::mutex m;
  std::map<int, DeviceScratch *> scratch;
  DeviceScratch *scratch_for(int device) {
    std::lock_guard<std::mutex> lk(m);
    DeviceScratch *&p = scratch[device];
    if (!p) p = new DeviceScratch();
    return p;
  }
  ~tq_ctx() {
    for (auto &kv : scratch) {
      (void)hipSetDevice(kv.first);
      if (kv.second->ev_last) (void)hipEventDestroy(kv.second->ev_last);
      kv.second->partials.release();
      kv.second->share_stage.release();
      kv.second->ashare_stage.release();
      kv.second->bshare_stage.release();
      delete kv.second;
    }
  }
};

struct tq_segment {
  tq_ctx *ctx = nullptr;
  int device = 0;
  hipStream_t stream = nullptr;
  uint32_t max_doc = 0;
  uint8_t record_option = 0;
  std::vector<uint8_t> h_idx, h_pos;  // host copies (empty for a device-resident upload)
  size_t idx_len = 0, pos_len = 0;    // sizes of the sub-files in HBM
  TqpInfo *d_tp_info = nullptr;       // device-side prepare: result slots (info + positions result)
  uint8_t *d_idx = nullptr, *d_pos = nullptr, *d_fn = nullptr, *d_alive = nullptr;
  // Multi-field segments (tq_segment_upload_fields): the fields' sub-files lie end to end in d_idx / d_pos (h_idx /
  // h_pos), field f's .idx sub-file (header included) at field_idx_base[f], its .pos sub-file at field_pos_base[f]; a
  // term's offsets are shifted by them when it is prepared (term_by_off is keyed by the shifted offset: one key per
  // (field, postings_off)).  d_fn is field 0's fieldnorms, d_fn_field[f] those of field f >= 1 (null: constant id).
  uint32_t n_fields = 1;
  uint64_t field_idx_base[TQ_MAX_FIELDS] = {}, field_idx_len[TQ_MAX_FIELDS] = {};
  uint64_t field_pos_base[TQ_MAX_FIELDS] = {}, field_pos_len[TQ_MAX_FIELDS] = {};
  uint8_t *d_fn_field[TQ_MAX_FIELDS] = {};
  uint32_t n_field_terms = 0;  // prepared terms of fields != 0 (0: no entry point looks at a query's handles for fields)
  uint8_t prep_field = 0;      // the field of the terms being registered (set under the lock by the field entry points)
  float *d_local_cache = nullptr;  // Bm25Weight.cache under the segment's OWN average fieldnorm (256 floats; null:
                                   // the header holds no usable token count): what the range maxima are built under
  uint64_t *d_docmat = nullptr;  // doc-major matrix of the dense lists (TqdSegment::docmat)
  uint64_t *d_doccls = nullptr;  // tf classes of the first TQD_CLS_SLOTS column lists (TqdSegment::doccls)
  uint32_t n_mat_slots = 0;
  TqdSegment dseg{};
  std::vector<TermHost> terms;
  std::vector<std::pair<void *, size_t>> rdir_chunks;  // the range directories' chunks (rdir_alloc, tq_term_arena.cpp)
  uint8_t *rdir_chunk_cur = nullptr;
  size_t rdir_chunk_left = 0;
  bool rdir_span_ok = false;       // ... all within the 32 GB the shared launches' table offsets reach (tq_search.cpp)
  std::vector<void *> term_slabs;  // the terms' table blobs are carved out of 4 MB slabs (term_alloc)
  uint8_t *term_slab_cur = nullptr;
  size_t term_slab_left = 0;
  std::vector<TqdTerm> h_dterms;
  TqdTerm *d_terms = nullptr;
  size_t d_terms_cap = 0;
  bool d_terms_dirty = false;
  size_t d_terms_dirty_from = ~(size_t)0;  // the lowest term record changed since the last sync
  size_t d_terms_synced = 0;               // records the device table holds (and batches in flight may read)
  size_t dense_bytes_total = 0;
  // The side tables of the dense lists (bitmaps + rank directories, byte-wide tfs, position directories,
  // plain lists) live in ONE device allocation of dense_budget() bytes, made with the first of them:
  // the term-major launches address them as 32-bit offsets (8-byte units) from its base.  (With one
  // hipMalloc per table the allocator now and then returned addresses more than 32 GB apart and the
  // launches silently fell back to the per-query kernels.)  What does not fit falls back to hipMalloc.
  uint8_t *dense_arena = nullptr;
  size_t dense_arena_cap = 0, dense_arena_used = 0;
  std::vector<void *> dense_extra;  // tables allocated outside the arena
  // Round 6: the arena is a RESERVED ADDRESS RANGE (hipMemAddressReserve, 24 GB of addresses — no memory), mapped
  // chunk by chunk as tables are added (hipMemCreate / hipMemMap): whatever the process has allocated and freed before,
  // every table of the segment lies within the 32 GB the shared launches' and the tree kernel's 32-bit table offsets
  // reach.  (A soak that opened and closed 230 indexes in one process got an overflow allocation more than 32 GB from
  // its arena: flat queries fell back to the per-query kernels, a nested query was refused.)  dense_arena_cap = the
  // reservation, dense_arena_mapped = what is backed by memory.  If the driver refuses any step: the old arena.
  bool dense_arena_vmm = false;
  void *dense_arena_va = nullptr;  // the reservation as the driver returned it (the arena starts at its first 32 MB multiple)
  size_t dense_arena_mapped = 0, dense_arena_first = 0;
  std::vector<std::pair<hipMemGenericAllocationHandle_t, size_t>> dense_arena_chunks;
  // resident bytes by kind (tq_segment_get_stats)
  size_t bytes_term_tables = 0, bytes_bitmaps = 0, bytes_docmat = 0, bytes_posdir = 0, bytes_alive = 0;
  uint32_t n_dense_lists = 0;
  // term sets (tq_termset.cpp): slots of `terms` that are or were sets (0: no entry point looks for them), the released
  // slots and tables a later set takes, the build's work lists and scan scratch
  uint32_t n_set_slots = 0;
  std::vector<uint32_t> set_free_slots;
  std::vector<void *> set_free_tables;
  DevBuf d_set_work;
  // fast-field columns (tq_column.cpp): u64_based column-values payloads as the file holds them, TQ_MAX_COLUMNS slots (a
  // released slot is taken by the next upload); tq_range_prepare makes term-set slots of them
  struct ColumnHost {
    bool live = false;
    tq_column_info_t info{};
    TqkColumn dev{};            // payload / blocks / present point into the three allocations below
    void *d_payload = nullptr;  // the codec's payload + 16 zero bytes
    void *d_blocks = nullptr;   // BlockwiseLinear: TqkColBlock per block
    void *d_present = nullptr;  // TQ_CARD_OPTIONAL: {presence bits, rows before the word}, n_words + 1 entries
    uint64_t payload_len = 0;
  };
  ColumnHost columns[TQ_MAX_COLUMNS];
  uint32_t alive_docs = 0;  // docs below max_doc the alive bitset keeps (counted when it is set; without one: max_doc)
  std::unordered_map<uint64_t, uint32_t> term_by_off;
  // lists named by tq_segment_reserve_columns (postings_off): only they get doc-matrix columns
  std::unordered_map<uint64_t, bool> reserved_cols;
  bool cols_reserved = false;
  // batch scratch
  DevBuf d_stage, d_misc, d_thr, d_qmatches;
  DevBuf d_share_words;   // shared-union launch: per-query words
  DevBuf d_count_queries, d_count_out, d_count_bits, d_count_wgs;  // Count collector over bitmaps (tq_count.hip)
  // full doc sets (tq_docset.hip): descriptors, the (query, tile) tables of the scan, and the host variant's outputs
  DevBuf d_docset_queries, d_docset_counts, d_docset_offs, d_docset_partials, d_docset_starts, d_docset_docs;
  // ... with scores (tq_docset_score.hip): scoring descriptors, the batch's Bm25Weight caches, the host variant's scores
  DevBuf d_docset_squeries, d_docset_caches, d_docset_scores;
  DevBuf d_docset_trees;  // ... of phrases and nested queries (tq_docset_tree.hip): their TqdTreeQuery records
  // sort by fast field (tq_sort.hip): the queries' k, the slices' lists and counts, the host variant's rows
  DevBuf d_sort_ks, d_sort_partials, d_sort_slice_counts, d_sort_rows;
  PinnedBuf h_sort_ks;  // ... the queries' k on their way up
  DevBuf d_agg_rows;  // aggregations (tq_agg.hip): the host variant's records and bucket rows
  DevBuf d_agg_term_rows;  // terms aggregation (tq_agg_terms.hip): the batch's count rows, n_queries x n_keys
  DevBuf d_agg_range_starts;     // range aggregation (tq_agg_range.hip): the plan's starts, uploaded per call
  PinnedBuf h_agg_range_starts;  // ... on their way up
  PinnedBuf h_docset;  // descriptors + scatter work list on their way up
  size_t docset_scratch_bytes() const {
    return d_docset_queries.cap + d_docset_counts.cap + d_docset_offs.cap + d_docset_partials.cap + d_docset_starts.cap +
           d_docset_docs.cap + d_docset_squeries.cap + d_docset_caches.cap + d_docset_scores.cap +
           d_docset_trees.cap + d_sort_ks.cap + d_sort_partials.cap + d_sort_slice_counts.cap + d_sort_rows.cap + d_agg_rows.cap + d_agg_term_rows.cap +
           d_agg_range_starts.cap;
  }
  DevBuf d_ashare_words, d_bshare_words;  // shared-intersection launches (run next to the shared-union one)
  DeviceScratch *dscratch = nullptr;  // partial / result lists and staging lists: the device's (tq_ctx)
  // the shared-union launch addresses bitmaps / byte-wide tfs as 32-bit offsets (8-byte units) from
  // the lowest such table: usable while all of them lie within 32 GB of device addresses
  size_t share_span_terms = 0;  // number of terms the span was computed over
  uint64_t share_table_lo = 0;
  bool share_span_ok = true;
  bool lnorm_off = false;  // a leader-norm table came to lie outside that span (build_lnorm): no more of them are built
  // Leaders' doc-matrix words in posting order (TermHost::lmat_blob) are copies of doc-matrix words: every writer of the
  // matrix bumps docmat_epoch (docmat_written), a table is used only while its lmat_epoch equals it.  A stale table is
  // refilled — in place, on the batch's stream behind order_batch, so after every batch that may read it — only when
  // the epoch did not move since the previous batch was planned (docmat_epoch_planned): a stream that prepares terms
  // in every batch never refills.
  uint64_t docmat_epoch = 1, docmat_epoch_planned = 0;
  size_t lmat_bytes_total = 0;
  bool lmat_off = false;   // a table came to lie outside the span: no more of them are built
  uint32_t lmat_stale_skips = 0;  // leaders of the last planned batch whose table was stale and therefore not used
  uint32_t last_batch_queries = 0;
  // sloppy phrases (tq_phrase_slop.cpp): per query of the batch, candidate docs whose carried list went over the cap
  DevBuf d_slop_over;
  bool last_batch_slop = false;  // the last batch held a sloppy phrase: d_slop_over is its overflow words
  uint32_t slop_over_words = 0;  // queries of the caller's last search / doc-set / count batch: d_slop_over holds one word
                                 // for each when last_batch_slop (tq_last_batch_slop_overflows; else every word reads 0)
  std::vector<uint32_t> slop_over_host;  // ... as search_batch_host left them under CallOpts::defer_slop_verdict
  std::vector<uint32_t> last_query_kernel;  // option "record_query_kernels": TQ_KERNEL_* of every query of the last batch
  PinnedBuf h_stage, h_out;
  // timing: a ring of event quadruples, one per batch, so that pipelined batches (no host sync
  // between them) can all be timed; tq_last_batch_stats averages the batches since its last call
  static constexpr int kTimingRing = 16;
  hipEvent_t ev_stage_done = nullptr, ev_fork = nullptr, ev_join = nullptr;
  // The per-segment scratch (query descriptors, partial lists, threshold slots, counters, the
  // side stream) is shared by consecutive batches: work enqueued on another stream than the
  // previous batch's must first wait for that batch (ev_batch_done, recorded at its end).
  hipEvent_t ev_batch_done = nullptr;
  hipStream_t last_stream = nullptr;
  bool batch_in_flight = false;
  hipStream_t side_stream = nullptr;  // the launch groups of one batch run concurrently
  // The batch's staging blob goes up on a stream of its own, into one of two device buffers, while
  // the previous batch's kernels still run.
  // Measured with SDMA copies: step 5.19 -> 5.12 ms on 60-step runs and a steadier step time;
  // round 1's attempt (one buffer, blit copies) had lost 8 %
  hipStream_t copy_stream = nullptr;
  DevBuf d_stage_alt;                        // the second staging buffer (d_stage is the first)
  hipEvent_t ev_copy_done[2] = {nullptr, nullptr}, ev_buf_free[2] = {nullptr, nullptr};
  bool buf_used[2] = {false, false};
  uint64_t batches_enqueued = 0;
  hipEvent_t ev_t0[kTimingRing] = {}, ev_t1[kTimingRing] = {}, ev_k0[kTimingRing] = {},
             ev_k1[kTimingRing] = {};
  uint64_t batches_timed = 0, batches_reported = 0;
  bool stage_in_flight = false;
  double host_ms_sum = 0;   // host time inside tq_search_batch_device since the last stats call
  uint32_t host_ms_n = 0;
  unsigned long long *d_match_counter = nullptr;
  Options opt;
  size_t dense_budget() const { return (size_t)opt.dense_budget_x * (idx_len + pos_len + max_doc); }
  size_t probe_budget() const { return (size_t)opt.probe_budget_x * (idx_len + pos_len + max_doc); }
  size_t rdir_budget() const { return (size_t)opt.rdir_budget_x * (idx_len + pos_len + max_doc); }
  size_t rdir_bytes_total = 0;
  // tq_term_prepare_batch: the blobs of a batch's new terms on their way up (two buffers, an event each), and which
  // of the two events the next batch has to wait for (-1: none)
  PinnedBuf h_prep_stage[2];
  hipEvent_t ev_prep[2] = {nullptr, nullptr}, ev_prep_order = nullptr;
  bool prep_used[2] = {false, false};
  uint32_t prep_calls = 0;
  int prep_pending = -1;
  // the largest tf/(tf + norm) of every list whose range directory a tq_term_prepare_batch call built: written by the build
  // launch, copied into the call's pinned buffer behind the blobs; TermHost::rmax_list gets it once the call's event has
  // completed (prep_apply_lmax: no wait — until then the list's weight bounds it)
  std::vector<uint32_t> prep_lmax_handles[2];
  const uint32_t *prep_lmax_host[2] = {nullptr, nullptr};
  size_t probe_bytes_total = 0;
  bool probe_full = false;  // (kept for tq_set_option; the pool below evicts instead of latching)
  // Probe pool (round 6): the private tables of lists below "dense_ratio" live in equal SLOTS — [bitmap + rank
  // directory | tf bytes | position directory | range maxima] — "probe_budget_x" worth of them (at least one query's:
  // TQ_MAX_TERMS).  A list that needs tables when every slot is taken gets the slot of the list that was used longest
  // ago (by batch); slots touched by the batch being planned are never taken — a batch that names more such lists
  // than the budget holds grows the pool for good.  Before, the budget latched ("probe_full") and every later
  // query that named a new sparse list fell back or — nested boolean queries — failed.
  struct ProbeSlot {
    uint8_t *base = nullptr;
    uint32_t owner = 0xFFFFFFFFu;  // term handle, or none
    uint64_t last_batch = 0;
  };
  std::vector<ProbeSlot> probe_slots;
  size_t probe_slot_bytes = 0, probe_bm_bytes = 0, probe_tf_cap = 0, probe_dir_cap = 0, probe_rm_bytes = 0;
  uint64_t probe_batch = 1;        // sequence number of the batch being planned
  uint64_t probe_evictions = 0;
  uint64_t probe_replaced_batch = 0;  // ... and how many slots such candidates took over in it
  uint32_t probe_replaced_n = 0;
  uint64_t probe_no_room_batch = 0;  // the batch in which a shared-launch candidate found no slot to take
  bool probe_waited = false;       // this batch already waited for the batches in flight before reusing a slot
  bool device_prepare() const { return h_idx.empty() || opt.device_prepare != 0; }
  tq_batch_stats stats{};
  bool stats_pending = false;
  uint32_t stats_match_bytes = 1;  // what a match adds to algorithmic_bytes once d_match_counter is read: a fieldnorm
                                   // byte per scored doc, 4 bytes per doc of a doc-set batch on the device (9 with scores)
  // the pending batch is a sorted one (tq_search_sorted_batch*): d_match_counter[0..2] = matches, matches with a value, row
  // entries written, which tq_last_batch_stats turns into bytes (8 per valued match, 8 per match of an Optional column, 13
  // per entry); set or cleared wherever stats_pending is set.  An aggregation batch (tq_agg_batch*) is counted the same
  // way: it writes no row entries, and its records and bucket rows are already in stats.algorithmic_bytes
  bool stats_sorted = false, stats_sorted_optional = false;
  // ... a sub-aggregation (tq_agg_sub_batch*): d_match_counter[3..4] = bucketed docs with a value in the metric column,
  // bucketed docs (8 per valued one, 8 per bucketed doc of an Optional metric column); set beside stats_sorted
  bool stats_agg_metric = false, stats_agg_metric_optional = false;
  // ... a terms aggregation (tq_agg_terms_batch*): d_match_counter[3] = entries returned (12 bytes each); the same
  bool stats_agg_terms = false;
  // ... with a metric (tq_agg_terms_sub_batch*): d_match_counter[4] = counted docs with a value in the metric column,
  // [5] = counted docs; 40 more bytes per entry returned
  bool stats_agg_terms_sub = false;
  // ... with a histogram per key (tq_agg_terms_hist_batch*): d_match_counter[4] / [5] likewise for the histogram column;
  // its buckets + 1 (0: not such a call): 4 x buckets per entry returned
  uint32_t stats_agg_terms_hist_row = 0;
  // host planner scratch (launch groups, chunk tables): kept between batches so that planning a
  // batch does not start by page-faulting tens of megabytes of fresh vectors
  struct PlanScratch *plan = nullptr;
  // One call at a time works on a segment's state (term table, planner scratch, staging buffers):
  // every entry point takes this lock, so concurrent callers are serialised, not undefined.
  // (recursive: tq_count_batch -> tq_search_batch -> ...)
  std::recursive_mutex exec_m;
  // tq_submit / tq_wait / tq_search_one: single queries of concurrent callers, coalesced into batches
  struct SubmitQueue *submit = nullptr;
};

void tq_free_plan_scratch(PlanScratch *p);  // (defined next to the planner)
void tq_free_submit_queue(struct SubmitQueue *q);
struct SubmitQueue *tq_new_submit_queue();
#define TQ_SEGMENT_LOCK(seg) std::lock_guard<std::recursive_mutex> tq_exec_lock_((seg)->exec_m)

namespace tqi {

// A grow-only array of plain structs whose resize() leaves new elements uninitialised (the
// descriptors of a 10 000-query batch are 3 MB: std::vector::resize would zero them just before
// they are overwritten).
template <typename T>
class PodVec {
 public:
  PodVec() = default;
  PodVec(const PodVec &) = delete;
  PodVec &operator=(const PodVec &) = delete;
  PodVec(PodVec &&o) noexcept : p_(o.p_), n_(o.n_), cap_(o.cap_) { o.p_ = nullptr, o.n_ = o.cap_ = 0; }
  PodVec &operator=(PodVec &&o) noexcept {
    swap(o);
    return *this;
  }
  ~PodVec() { free(p_); }
  size_t size() const { return n_; }
  bool empty() const { return n_ == 0; }
  T *data() { return p_; }
  const T *data() const { return p_; }
  T &operator[](size_t i) { return p_[i]; }
  const T &operator[](size_t i) const { return p_[i]; }
  T &back() { return p_[n_ - 1]; }
  const T &back() const { return p_[n_ - 1]; }
  T *begin() { return p_; }
  T *end() { return p_ + n_; }
  const T *begin() const { return p_; }
  const T *end() const { return p_ + n_; }
  void clear() { n_ = 0; }
  void reserve(size_t n) {
    if (n <= cap_) return;
    const size_t ncap = std::max(n, cap_ * 2);
    T *np = (T *)malloc(ncap * sizeof(T));
    if (!np) throw std::bad_alloc();
    if (n_) memcpy(np, p_, n_ * sizeof(T));
    free(p_);
    p_ = np;
    cap_ = ncap;
  }
  void resize(size_t n) {  // (new elements are NOT initialised)
    reserve(n);
    n_ = n;
  }
  void push_back(const T &v) {
    if (n_ == cap_) reserve(n_ + 1);
    p_[n_++] = v;
  }
  void append(const T *first, const T *last) {
    const size_t n = (size_t)(last - first);
    reserve(n_ + n);
    if (n) memcpy(p_ + n_, first, n * sizeof(T));
    n_ += n;
  }
  void swap(PodVec &o) {
    std::swap(p_, o.p_);
    std::swap(n_, o.n_);
    std::swap(cap_, o.cap_);
  }

 private:
  T *p_ = nullptr;
  size_t n_ = 0, cap_ = 0;
};

struct Group {
  int mode;
  PodVec<TqdQuery> queries;
  std::vector<uint32_t> out_index;
  std::vector<uint32_t> tile_starts;
  std::vector<uint4> chunk_recs;      // launch order: {first tile, end tile, first query, chunk}
  std::vector<uint32_t> tile_cost;  // per query, cost units per tile
  std::vector<TqdTreeQuery> tree;   // kGTree: the nested boolean queries' descriptors (tq_tree.hip), one per query
  std::vector<TqdAllQuery> all;     // kGAll: the ALL-BASED queries' descriptors (tq_all.hip), one per query
  std::vector<TqdSlopQuery> slop;   // kGSlop: the sloppy phrases' descriptors (tq_phrase_slop.hip), one per query
  uint32_t total_tiles = 0, n_chunks = 0, max_k = 1;
  uint64_t list_entries = 0;  // term-major / doc-major groups: 8-byte entries of the group's result lists
  int kpl = 1;
  // offsets inside the staging blob
  size_t o_queries = 0, o_tiles = 0, o_outidx = 0, o_chunks = 0, o_sinks = 0;
  size_t o_xqueries = 0;  // (shared intersections) the full records of the queries with three and more lists
  size_t o_leads = 0, o_tasks = 0, o_lists = 0;  // the extra tables of the shared, doc-major and tree groups
  void reset() {  // keeps the vectors' capacity
    queries.clear();
    out_index.clear();
    tile_starts.clear();
    chunk_recs.clear();
    tile_cost.clear();
    tree.clear();
    all.clear();
    slop.clear();
    total_tiles = 0;
    n_chunks = 0;
    list_entries = 0;
    max_k = 1;
    kpl = 1;
    o_queries = o_tiles = o_outidx = o_chunks = o_sinks = o_xqueries = 0;
    o_leads = o_tasks = o_lists = 0;
  }
};

}  // namespace tqi

struct alignas(128) PlanSlab {  // chunk tables of one slab of queries (build_group_chunks); its own
                                // cache lines: the slabs' vector ends are bumped by different threads
  size_t q0 = 0, q1 = 0;
  std::vector<uint32_t> starts, slice, query;
};
struct ALeadKey {  // sort key of one lead of the shared-intersection group
  uint64_t k1;    // leader handle << 8 | cache
  uint64_t mask;  // doc-matrix bits of the other lists
  uint64_t sig;   // hash of the whole query (lists, weights, k): identical queries become neighbours
  uint32_t q, pad;
};
// (the shared-intersection planner orders the leads of one (leader, cache) by this bin of their mask: leads with the
// same mask are neighbours, two masks in one bin — 2 048 bins — may interleave; tools/planbench/plan_check.cpp)
constexpr uint32_t kALeadMaskBins = 2048;
inline uint32_t alead_mask_bin(uint64_t m) { return (uint32_t)((m * 0x9E3779B97F4A7C15ull) >> 53); }
struct ShareKey {  // one (query, list) pair of the shared-union group
  uint64_t key;    // list position i << 56 | blocks of the term (rare terms first) << 32 | cache
  uint32_t term, q;
};
// The launch groups of a batch.  The values are also the order of the groups' partial lists in the batch's buffer,
// so they stay as they are.
enum GroupId : int {
  kGAndDense = 0,  // AND queries whose non-leader lists all have a bitmap (and_kernel's lean instantiation)
  kGUnion = 1,     // unions (candidate-driven per query, or 4096-doc windows)
  kGPhrase = 2,    // phrases
  kGAnd = 3,       // AND queries over any lists
  kGBool = 4,      // boolean queries (clauses with roles: the union kernel's BOOL instantiation)
  kGUShare = 5,    // shared unions (term-major for the batch, tq_ushare.hip)
  kGPhSweep = 6,   // phrases through the bitmap-AND sweep
  kGXUnion = 7,    // unpruned unions, doc-major for the batch (tq_xunion.hip)
  kGAShare = 8,    // shared intersections (leader-major for the batch, tq_ashare.hip)
  kGBShare = 9,    // boolean queries through the shared-intersection launch
  kGTree = 10,     // nested boolean queries over bitmaps (tq_tree.hip)
  kGAll = 11,      // ALL-BASED queries (TQ_TERM_ALL clauses) over bitmaps (tq_all.hip)
  kGSlop = 12,     // TQ_MODE_PHRASE with slop > 0 over bitmaps (tq_phrase_slop.hip)
  kNGroups = 13
};
// per group: the TQ_MODE_* of its descriptors; whether it writes result lists (part_start / n_parts count 8-byte
// entries) rather than per-tile partials; its TQ_KERNEL_* bit (the union group's: group_kernel_bit)
struct GroupTraits { int mode; bool result_lists; uint32_t kernel; };
constexpr GroupTraits kGroupTraits[kNGroups] = {
    {TQ_MODE_AND, false, TQ_KERNEL_AND_DENSE}, {TQ_MODE_OR, false, TQ_KERNEL_UNION}, {TQ_MODE_PHRASE, false, TQ_KERNEL_PHRASE},
    {TQ_MODE_AND, false, TQ_KERNEL_AND},       {TQ_MODE_OR, false, TQ_KERNEL_BOOL},  {TQ_MODE_OR, true, TQ_KERNEL_USHARE},
    {TQ_MODE_PHRASE, false, TQ_KERNEL_PHRASE_SWEEP}, {TQ_MODE_OR, true, TQ_KERNEL_XUNION}, {TQ_MODE_AND, true, TQ_KERNEL_ASHARE},
    {TQ_MODE_OR, true, TQ_KERNEL_BSHARE},      {TQ_MODE_OR, false, TQ_KERNEL_TREE},
    {TQ_MODE_OR, false, TQ_KERNEL_ALL},        {TQ_MODE_OR, false, TQ_KERNEL_PHRASE_SLOP}};
inline uint32_t group_kernel_bit(int gi, bool or_windows) {
  return gi == kGUnion && or_windows ? TQ_KERNEL_OR_WINDOWS : kGroupTraits[gi].kernel;
}
struct RouteTotals {  // what routing a run of queries adds up besides the groups' descriptors
  uint32_t n_thr_rows = 0;
  uint32_t n_ashare_ext = 0;  // shared intersections of three and more lists (their full records ride in a side array)
  uint64_t algo_bytes = 0;
  bool phrase_all_dense = true;  // (the phrase group may run the lean instantiation)
};
struct QuerySlab {  // one slab of a batch's queries, planned by one thread into groups of its own
  Group groups[kNGroups];
  RouteTotals t;
  int rc = 0;
  std::string err;
};
struct PlanScratch {
  Group groups[kNGroups];
  std::vector<uint32_t> q_cache;      // per query of the batch: its Bm25Weight cache
  std::vector<QuerySlab> q_slabs;
  // doc-major union group (tq_xunion.hip): the lists of the batch (<-> rows of the tile), the queries
  std::vector<TqkDenseRow> xrows;
  std::vector<TqkDenseQuery> xqueries;
  std::vector<uint64_t> xrow_term;           // row -> term handle << 32 | weight bits, in order of first use
  std::unordered_map<uint64_t, uint32_t> xrow_of;  // ... -> row
  uint32_t xcache = 0xFFFFFFFFu;  // the group's one Bm25Weight cache
  uint32_t xgrid = 0, x_bitmap_rows = 0, x_tiles_per_task = 1, x_list_stride = 0, x_max_terms = 1;
  // shared-union group (tq_ushare.hip): leads grouped by term, tasks in launch order
  std::vector<ShareKey> share_keys, share_keys2;
  std::vector<uint64_t> sort_keys, sort_keys2;
  std::vector<uint32_t> term_rank, term_distinct;
  std::vector<TqdLead> leads;
  std::vector<uint4> tasks;
  std::vector<uint32_t> share_pairs;  // per query: (task, lead) pairs = result-list appends at most
  // shared-intersection launches (tq_ashare.hip): [0] the AND group (one lead per query), [1] the boolean
  // group (one lead per (query, list of its lead set)); leads sorted by (leader, cache, mask, query hash)
  struct ASharePlan {
    std::vector<TqdALead> aleads, aleads_unsorted;
    std::vector<ALeadKey> alead_keys, alead_keys2;
    std::vector<uint32_t> alead_first, alead_bucket, alead_bucket_at, alead_bucket_starts;
    std::vector<uint8_t> alead_same;
    std::vector<uint64_t> aq_sig;   // per query of the group: hash of the whole query (lists, weights, k, roles)
    std::vector<uint64_t> aq_slot;  // open-addressing table over aq_sig: the first query with that content
    struct QKey {
      uint32_t t0, t1, w0, w1, k, shape;
    };
    std::vector<QKey> aq_key;
    std::vector<uint32_t> aowner;  // per query of the group: the query whose result list it reads (itself, or the identical query before it)
    std::vector<uint4> atasks;
    std::vector<uint2> alists;  // boolean group: [query][list] = {bitmap, tf bytes} as offsets from the table base
    std::vector<uint32_t> apairs, atask_hist, atask_slab_run;
    struct ARun {  // the leads of one (leader, cache)
      uint32_t r0, r1, term, cache, n_blocks, n_groups, per_group, bpt, nb_warm, n_runs;
      size_t task0;
    };
    std::vector<ARun> aruns;
    uint32_t a_warm_tasks = 0;  // tasks [0, a_warm_tasks) are the warm-up launch (band 1)
    // one dispatch for the whole launch (option "ashare_inline_warm"): the main tasks come in two bands — [a_warm_tasks,
    // a_dep_tasks) tasks of leaders WITHOUT warm-up tasks from the first doc slices, as many as the resident wavefronts
    // need, [a_dep_tasks, end) all the others — each in doc-slice order; false: one band, a_dep_tasks = a_warm_tasks
    bool a_inline = false;
    uint32_t a_dep_tasks = 0;
    bool over_budget = false;   // the last plan failed because its result lists exceed TQ_AS_LIST_MB at the longest tasks
    bool any_rdir = false;      // (boolean leads) some list of alists is probed through its range directory
  };
  ASharePlan ap[2];
  std::vector<uint32_t> q_leader;        // per query of the batch: the list that would lead it there, or 0xFFFFFFFF
  std::vector<uint32_t> and_lead_count;  // per term handle: AND queries of the batch it could lead in that launch
  std::vector<uint32_t> term_stamp;      // per term handle: last batch that used the list (unique bytes)
  uint32_t batch_stamp = 0;
  uint32_t share_phase_first[TQD_US_MAX_TERMS + 1];  // tasks of list position i: [first[i], first[i+1])
  uint64_t share_table_base = 0;  // TqdLead::dense_off / tf8_off are relative to this device address
  std::vector<uint32_t> lead_cost, sort_start;
  std::vector<PlanSlab> slabs;
  std::vector<std::pair<uint64_t, uint32_t>> keyed;
  PodVec<TqdQuery> q_tmp;
  std::vector<uint32_t> o_tmp, c_tmp, hist;
  std::vector<uint4> sorted_recs;
};

namespace tqi {

// Planner threads (TQ_PLAN_THREADS, default 4, 1 = off): the chunk tables of a large batch are
// built in slabs of queries / slices / records.  The helpers are a process-wide pool of detached
// threads that sleep on a condition variable between jobs (created on first use, never torn
// down: a batch plans in four parallel steps, and spawning threads for each of them cost more
// than the steps themselves — 2.1 ms of host time per 10 000-query AND batch against 1.3 ms for
// the same tables built by one thread).  One job at a time: a caller that finds the pool busy
// (another segment planning on another thread) runs its slabs itself.
uint32_t plan_threads();  // TQ_PLAN_THREADS (default 1: the calling thread alone)
class PlanPool {
 public:
  static PlanPool &get() {
    static PlanPool *pool = new PlanPool();  // (leaked on purpose: its threads outlive static destruction)
    return *pool;
  }
  // fn(ctx, slab) for slab in [0, n): the caller takes part, returns when all slabs are done
  void run(uint32_t n, void (*fn)(void *, uint32_t), void *ctx) {
    std::unique_lock<std::mutex> job_lock(job_mutex_, std::try_to_lock);
    if (!job_lock.owns_lock() || !ensure_workers(std::min<uint32_t>(n, plan_threads()) - 1u)) {
      for (uint32_t i = 0; i < n; ++i) fn(ctx, i);
      return;
    }
    uint64_t gen;
    {
      std::lock_guard<std::mutex> lk(m_);
      fn_ = fn;
      ctx_ = ctx;
      n_ = n;
      gen = generation_.load(std::memory_order_relaxed) + 1;
      done_.store(0, std::memory_order_relaxed);
      ticket_.store(gen << 32, std::memory_order_release);
      generation_.store(gen, std::memory_order_release);
    }
    cv_.notify_all();
    work(gen, fn, ctx, n);
    // (the slabs are short: spin for the last ones instead of sleeping)
    while (done_.load(std::memory_order_acquire) < n) std::this_thread::yield();
  }

 private:
  // Slabs are handed out through one word, generation << 32 | next slab: a helper that wakes up
  // late (its job already over, maybe the next one under way) finds another generation there and
  // takes nothing.
  void work(uint64_t gen, void (*fn)(void *, uint32_t), void *ctx, uint32_t n) {
    for (;;) {
      uint64_t cur = ticket_.load(std::memory_order_acquire);
      if ((cur >> 32) != (gen & 0xFFFFFFFFull) || (uint32_t)cur >= n) return;
      if (!ticket_.compare_exchange_weak(cur, cur + 1, std::memory_order_acq_rel)) continue;
      fn(ctx, (uint32_t)cur);
      done_.fetch_add(1, std::memory_order_release);
    }
  }
  bool ensure_workers(uint32_t want) {  // (under job_mutex_)
    while (n_workers_ < want) {
      try {
        std::thread([this] { worker(); }).detach();
        ++n_workers_;
      } catch (...) {  // a thread limit: plan with what there is
        break;
      }
    }
    return n_workers_ > 0;
  }
  void worker() {
    uint64_t seen = 0;
    for (;;) {
      void (*fn)(void *, uint32_t);
      void *ctx;
      uint32_t n;
      // a batch brings a dozen jobs within a millisecond: stay awake for a while after each one (a
      // wake-up through the condition variable costs 50-100 us, more than most of the jobs)
      const auto spin_until = std::chrono::steady_clock::now() + std::chrono::microseconds(400);
      while (generation_.load(std::memory_order_acquire) == seen && std::chrono::steady_clock::now() < spin_until)
#if defined(__x86_64__) || defined(__i386__)
        __builtin_ia32_pause();
#else
        std::this_thread::yield();
#endif
      {
        std::unique_lock<std::mutex> lk(m_);
        cv_.wait(lk, [&] { return generation_.load(std::memory_order_relaxed) != seen; });
        seen = generation_.load(std::memory_order_relaxed);
        fn = fn_;
        ctx = ctx_;
        n = n_;
      }
      work(seen, fn, ctx, n);
    }
  }
  std::mutex job_mutex_, m_;
  std::condition_variable cv_;
  void (*fn_)(void *, uint32_t) = nullptr;
  void *ctx_ = nullptr;
  uint32_t n_ = 0, n_workers_ = 0;
  std::atomic<uint64_t> generation_{0};
  std::atomic<uint64_t> ticket_{0};
  std::atomic<uint32_t> done_{0};
};
template <typename F>
void parallel_slabs(uint32_t n_slabs, F &&fn) {  // fn(slab) for slab in [0, n_slabs)
  if (n_slabs <= 1) {
    if (n_slabs) fn(0u);
    return;
  }
  PlanPool::get().run(
      n_slabs, [](void *c, uint32_t i) { (*static_cast<typename std::remove_reference<F>::type *>(c))(i); }, (void *)&fn);
}

// stable sort of a handful of items (<= TQ_MAX_TERMS): std::stable_sort allocates a buffer per call,
// which was a quarter of the per-query planning time of a 10 000-query batch
template <typename T, typename Less>
inline void small_stable_sort(T *first, T *last, Less less) {
  for (T *i = first + (first != last); i < last; ++i) {
    T v = *i;
    T *j = i;
    while (j > first && less(v, j[-1])) {
      *j = j[-1];
      --j;
    }
    *j = v;
  }
}

inline int kpl_for(uint32_t k) { return k <= 64 ? 1 : (k <= 128 ? 2 : (k <= 256 ? 4 : 16)); }

inline uint64_t xrow_key(uint32_t term, float w) {
  uint32_t wb;
  memcpy(&wb, &w, sizeof wb);
  return ((uint64_t)term << 32) | wb;
}
// Per-call execution options (tq_search_opts resolved against the segment's defaults): nothing
// a call needs is read from mutable segment state after this point.
struct CallOpts {
  bool exhaustive;
  float bound_slack;
  bool no_ashare = false, no_bshare = false;  // (internal) this call keeps intersections / boolean queries off the shared launch
  // (internal) pinned host words, one per query: where a batch that holds a sloppy phrase copies its overflow words
  // behind its last kernel (tq_phrase_slop.cpp); a batch without one leaves them alone (tq_segment::last_batch_slop)
  uint32_t *h_slop_over = nullptr;
  // (internal, search_batch_host) a sloppy phrase over the carry cap is not an error of the call: the overflow words are
  // left in tq_segment::slop_over_host for the caller to judge (tq_submit: only that query's ticket fails)
  bool defer_slop_verdict = false;
};
// ---- tq_api.cpp: the segment's stream
int order_after_last_batch(tq_segment *s, hipStream_t st);
int wait_segment_idle(tq_segment *s);
// ---- tq_terms.cpp
// the handle of a new term: its records appended to the host tables (the five facts every preparation path registers)
uint32_t add_term(tq_segment *s, const TqdTerm &dt, const TermHost &th, uint64_t postings_off);
int register_term(tq_segment *s, const TqdTerm &dt, const TermHost &th, uint64_t postings_off, tq_term_handle *out);
int term_prepare_shifted(tq_segment *s, uint64_t postings_off, uint32_t postings_len, uint64_t positions_off,
                         uint32_t positions_len, uint32_t doc_freq, tq_term_handle *out);
int term_prepare_batch_shifted(tq_segment *s, const tq_term_info *infos, uint32_t n, tq_term_handle *out, uint8_t field);
int sync_terms(tq_segment *s, hipStream_t st);
void mark_term_dirty(tq_segment *s, uint32_t handle);
// a TermInfo's postings range lies inside the idx sub-file's body (idx_len counts its 8-byte header)
inline bool postings_range_ok(size_t idx_len, uint64_t off, uint32_t len) {
  return off <= idx_len - 8 && (uint64_t)len <= idx_len - 8 - off;
}
inline int bad_postings_range(size_t idx_len, uint64_t off, uint32_t len) {
  return fail(TQ_ERR_FORMAT, "postings_range [%llu,+%u) outside the idx body (%zu)", (unsigned long long)off, len, idx_len - 8);
}
// "this list is dense enough for tables of its own" (0.25 B/doc per bitmap: worth it for lists whose 128-doc blocks
// span few docs) ... and only while the side tables together stay within the budget (dense_fits: under the lock)
inline size_t bitmap_words(const tq_segment *s) { return ((size_t)s->max_doc + 31) / 32 + 1; }
inline size_t dense_table_bytes(const tq_segment *s) { return bitmap_words(s) * sizeof(uint2); }
inline bool dense_candidate(const tq_segment *s, uint32_t doc_freq) {
  return s->opt.dense && s->max_doc >= 4096u && (uint64_t)doc_freq * (uint64_t)s->opt.dense_ratio >= s->max_doc;
}
inline bool dense_fits(const tq_segment *s) { return s->dense_bytes_total + dense_table_bytes(s) <= s->dense_budget(); }
// ---- tq_term_walk.cpp: pure host code
struct WalkSource {  // what the walker reads of a segment
  const uint8_t *idx;  // the idx sub-file (8-byte header + body) and the pos sub-file (pos_len 0: none)
  size_t idx_len;
  const uint8_t *pos;
  size_t pos_len;
  uint8_t record_option;
  uint32_t max_doc;
};
inline WalkSource walk_source(const tq_segment *s) {
  return {s->h_idx.data(), s->h_idx.size(), s->h_pos.data(), s->h_pos.size(), s->record_option, s->max_doc};
}
inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }
// A term's blob: block records (+ the terminator), coarse table, tail docs / tfs, position-block table, position
// tail (both empty: no positions part), the term's own record — each 16-byte aligned — and PAD.
struct TermBlobLayout {
  size_t o_rec = 0, o_coarse = 0, o_tdocs = 0, o_ttfs = 0, o_pboff = 0, o_ptail = 0, o_self = 0, total = 0;
};
TermBlobLayout term_blob_layout(uint32_t n_blocks, uint32_t n_buckets, uint32_t n_tail, uint32_t n_pos_blocks, uint32_t n_pos_tail);
// coarse[b] = first block whose last doc >= b << shift, about one block per bucket: the shift, *n_buckets
uint32_t coarse_shift(uint32_t max_doc, uint32_t n_blocks, uint32_t *n_buckets);
// What the host walk of one posting list leaves: the bytes of the term's blob and everything of its records but the
// device pointers.
struct WalkedTerm {
  std::vector<uint8_t> hb;
  TermBlobLayout lay;
  TqdTerm dt{};
  TermHost th;
  uint64_t postings_off = 0;
};
int host_walk_term(const WalkSource &src, uint64_t postings_off, uint32_t postings_len, uint64_t positions_off,
                   uint32_t positions_len, uint32_t doc_freq, WalkedTerm &w);
void place_walked_term(WalkedTerm &w, uint8_t *blob);  // the device pointers of a walked term whose blob lives at `blob`
const char *tqp_message(uint32_t st);
// ---- tq_term_arena.cpp
int term_alloc(tq_segment *s, size_t bytes, uint8_t **out);
void term_release(tq_segment *s, uint8_t *blob, size_t bytes);
int dense_alloc(tq_segment *s, size_t bytes, void **out);
void dense_release(tq_segment *s, void *ptr);
void dense_arena_free(tq_segment *s);  // (the arena of the dense lists' side tables — a hipMalloc or a mapped address range)
int rdir_alloc(tq_segment *s, size_t bytes, void **out);
// ---- tq_term_tables.cpp
// A list decoded into the segment's d_misc: doc ids, term freqs, then scratch for the scans and the range maxima's
// accumulators (null: not asked for).
struct DecodedList {
  uint32_t *dd = nullptr, *dt = nullptr, *scan_scratch = nullptr, *rm_acc = nullptr;
};
int decode_list(tq_segment *s, const TermHost &t, size_t scan_words, bool want_rm, DecodedList &dl);
// enqueue: bitmap + rank directory of a decoded list into `blob` (validity flag: d_tp_info); its range maxima into `out`;
// then wait and read back the flag / the list's maximum (null: not wanted)
hipError_t enqueue_bitmap(tq_segment *s, const DecodedList &dl, uint32_t doc_freq, void *blob);
hipError_t enqueue_rmax(tq_segment *s, const DecodedList &dl, uint32_t doc_freq, uint8_t *out);
hipError_t finish_tables(tq_segment *s, const DecodedList &dl, uint32_t *bad, uint32_t *lmax);
inline uint32_t rmax_list_of(uint32_t lmax) { return lmax ? std::min<uint32_t>(lmax, 255u) : 255u; }
inline uint32_t sig_bit(uint32_t handle) { return (handle * 0x9E3779B1u) >> (32 - 4); }  // 0 .. TQD_SIG_BITS - 1
uint32_t rdir_plan(tq_segment *s, uint32_t doc_freq);
size_t rdir_dir_words(const tq_segment *s, uint32_t S);                  // directory slots of a shift, padded to four
size_t rdir_bytes(const tq_segment *s, uint32_t doc_freq, uint32_t S);  // ... + one entry per posting, in bytes
int attach_rdir(tq_segment *s, uint32_t handle, uint32_t S, void **tab);  // allocates the list's range directory and names it in its TermHost
int ensure_docmat(tq_segment *s);
int add_to_doc_signatures(tq_segment *s, uint32_t handle);
int build_dense_device(tq_segment *s, uint32_t handle);
int build_flat(tq_segment *s, uint32_t handle, hipStream_t st, bool *ok);
void build_lnorm(tq_segment *s, uint32_t handle, hipStream_t st);
// the doc matrix has been (or is being) written: tables copied out of it are stale
inline void docmat_written(tq_segment *s) { ++s->docmat_epoch; }
// (experiments: TQ_LEAD_MAT_BUDGET_X / TQ_LEAD_MAT_CUT override the options "lead_mat_budget_x" / "lead_mat_cut")
inline int lead_mat_budget_x(const tq_segment *s) {
  static const uint32_t kEnv = tune_u32("TQ_LEAD_MAT_BUDGET_X", 0xFFFFFFFFu);
  return kEnv != 0xFFFFFFFFu ? (int)std::min<uint32_t>(kEnv, 0x7FFFFFFFu) : s->opt.lead_mat_budget_x;
}
inline uint32_t lead_mat_cut(const tq_segment *s) {
  static const uint32_t kEnv = tune_u32("TQ_LEAD_MAT_CUT", 0);
  return kEnv ? kEnv : (uint32_t)std::max(1, s->opt.lead_mat_cut);
}
inline bool lmat_valid(const tq_segment *s, const TermHost &t) {
  return t.lmat_blob && t.lmat_epoch == s->docmat_epoch && lead_mat_budget_x(s) > 0;
}
// true: the list has a table this batch may name; *fill: ... once fill_lmat has run for it on the batch's stream
bool plan_lmat(tq_segment *s, uint32_t handle, bool *fill);
hipError_t fill_lmat(tq_segment *s, uint32_t handle, hipStream_t st);
void prep_apply_lmax(tq_segment *s, bool wait);    // rmax_list of lists prepared by finished tq_term_prepare_batch calls
// ---- tq_term_probe.cpp
// must: the caller cannot run without the tables (nested boolean queries): any segment size, the least recently used
// slot if none is free; else: only a free slot or one idle for a while
int build_probe_tables(tq_segment *s, uint32_t handle, bool *ok, bool must = false);
int build_probe_posdir(tq_segment *s, uint32_t handle, bool *ok);
void probe_begin_batch(tq_segment *s);             // a new batch is being planned (the pool's clock)
void probe_touch(tq_segment *s, uint32_t handle);  // the batch being planned uses the list's probe tables
// ---- tq_all.cpp: AllQuery clauses (TQ_TERM_ALL), the normal form of a flat query that holds them
inline bool query_has_all(const tq_query &q) {
  if (!q.terms || q.n_terms > TQ_MAX_TERMS) return false;
  for (uint32_t i = 0; i < q.n_terms; ++i)
    if (q.terms[i] == TQ_TERM_ALL) return true;
  return false;
}
struct AllForm {
  uint32_t kind = TQ_ALL_EMPTY;  // enum tq_all_kind
  float base = 0.0f;
  uint32_t min_should = 0, keep_mask = 0;
  bool boost_mixed = false;  // a boosted All beside another scoring clause or a second All: doc sets only
};
// TQ_OK, or TQ_ERR_INVALID / TQ_ERR_UNSUPPORTED with *why (the caller names the query)
int all_query_form(const tq_query &q, AllForm &f, const char **why);
struct AllView {  // the entries of keep_mask as a query of their own (borrows q's tf_cache); EMPTY: one absent Must term
  tq_query q;
  tq_term_handle terms[TQ_MAX_TERMS];
  float weights[TQ_MAX_TERMS];
  uint8_t occurs[TQ_MAX_TERMS], clause_of[TQ_MAX_TERMS];
  uint32_t pos[TQ_MAX_TERMS];  // where entry i of the view stands in the caller's query
};
void all_strip_view(const tq_query &q, const AllForm &f, AllView &v);
// ---- tq_termset.cpp: term sets (tq_term_set_prepare: a slot of the term table that is a bitmap and scores a constant)
inline bool is_term_set(const tq_segment *s, uint32_t h) { return h < s->terms.size() && s->terms[h].set_kind == TermHost::kSet; }
// a set's table: (max_doc / 32 words + the sentinel) from the released tables or the arena; back to them; and the slot of
// the term table that makes a BUILT table a set of n_docs docs (tq_range_prepare's handles are such slots too)
int set_table_acquire(tq_segment *s, void **tab);
void set_table_release(tq_segment *s, void *tab);
uint32_t set_slot_commit(tq_segment *s, void *tab, uint32_t n_docs);
void free_columns(tq_segment *s);  // tq_column.cpp: the fast-field columns still held (tq_segment_free)
// a list's bitmap as the count / doc-set expressions name it: its own where "use_dense" allows, a set's always (it has nothing else)
inline const void *expression_bitmap(const tq_segment *s, const TermHost &th) {
  return th.dense_blob && (s->opt.use_dense || th.set_kind == TermHost::kSet) ? th.dense_blob : nullptr;
}
// ---- multi-field segments: does the query name a list of a field != 0?  (Asked only while s->n_field_terms != 0.)
static_assert(TQK_MAX_FIELDS == TQ_MAX_FIELDS, "the multi-field launch parameters hold one fieldnorm pointer per field");
inline uint32_t term_field_of(const tq_segment *s, uint32_t h) { return h < s->terms.size() ? s->terms[h].field : 0u; }
inline bool query_names_field(const tq_segment *s, const tq_query &q) {
  if (!q.terms || q.n_terms > TQ_MAX_TERMS) return false;
  for (uint32_t i = 0; i < q.n_terms; ++i)
    if (term_field_of(s, q.terms[i])) return true;
  return false;
}
// The field of the terms registered while the scope — and the segment's lock — is held: add_term tags them with it.
struct FieldScope {
  tq_segment *s;
  uint8_t was;
  FieldScope(tq_segment *seg, uint8_t field) : s(seg), was(seg->prep_field) { s->prep_field = field; }
  ~FieldScope() { s->prep_field = was; }
  FieldScope(const FieldScope &) = delete;
  FieldScope &operator=(const FieldScope &) = delete;
};
// TQ_ERR_INVALID (`fn: query qi: ...`) for a phrase, or a phrase atom, whose present terms are of different fields
int check_field_query(const tq_segment *s, const tq_query &q, uint32_t qi, const char *fn);
inline bool query_names_set(const tq_segment *s, const tq_query &q) {
  if (!q.terms || q.n_terms > TQ_MAX_TERMS) return false;
  for (uint32_t i = 0; i < q.n_terms; ++i)
    if (is_term_set(s, q.terms[i])) return true;
  return false;
}
// Does the query name a set?  (*has; false at once while the segment has never had one.)  TQ_ERR_INVALID: it names a
// released set, or a set in a phrase; TQ_ERR_UNSUPPORTED: a set inside a nested query — `fn: query qi: ...` either way.
int check_set_query(const tq_segment *s, const tq_query &q, uint32_t qi, const char *fn, bool *has);
// ---- tq_count.cpp
int count_batch(tq_segment *s, const tq_query *queries, uint32_t n_queries, uint32_t *out_counts);
// a query as a bitwise expression over bitmap words (tq_count.cpp; checked on the CPU by tools/planbench/plan_check.cpp)
bool count_expression(tq_segment *s, const tq_query &q, TqkCountQuery &cq, bool &known, uint64_t &driver_postings,
                      std::unordered_map<uint32_t, uint32_t> &temp_slot, uint32_t max_temp);
// the clauses of a flat query: what count_expression and docset_expression start from
struct FlatClauses {
  struct Clause {
    uint32_t id, occur, n = 0, terms[TQ_MAX_TERMS];
    uint32_t pos[TQ_MAX_TERMS];  // where terms[i] stands in tq_query.terms (its weight)
    uint64_t cost = 0;
  };
  Clause cl[TQ_MAX_TERMS];
  uint32_t n_cl = 0, n_must = 0, n_should = 0;  // (n_should: the Should clauses that hold a list)
  bool empty = false;                           // a Must clause without a list: no doc matches
  uint32_t msm = 0;                             // minimum_number_should_match (a query with All clauses: what they left of it)
  // BooleanWeight::complex_scorer (boolean_weight.rs:236-431): no list can match / all of the Should clauses are wanted: Must clauses
  bool empty_set() const { return !all_based && (empty || msm > n_should || (n_must == 0 && n_should == 0)); }
  bool should_is_must() const { return !all_based && msm >= 2 && msm == n_should; }
  // a query with All clauses that came out ALL-BASED (tq_all.cpp): the Should and MustNot clauses above, over every doc
  bool all_based = false, all_boost_mixed = false;
  float all_base = 0.0f;
};
enum { FLAT_OK = 0, FLAT_UNSUPPORTED, FLAT_INVALID };
int parse_flat_clauses(tq_segment *s, const tq_query &q, FlatClauses &fc, const char **why);
// ---- tq_docset.cpp: full doc sets (tq_docset_batch* / tq_docset_scored_batch*) and what else consumes their match words
// the query as a TqkDocsetQuery: FLAT_*; lists without a bitmap are left as their term HANDLE in dq.dense (narrow bit set);
// fc_out (or null): the clauses it was made from
int docset_expression(tq_segment *s, const tq_query &q, TqkDocsetQuery &dq, const char **why, FlatClauses *fc_out = nullptr);
// the scoring lists of the same query in summation order (weights and access paths; cache_idx is left to the caller)
void score_expression(tq_segment *s, const tq_query &q, const FlatClauses &fc, TqkScoreQuery &sq);
// Sort by fast field (tq_sort.cpp): the selection launch(es) of tq_sort.hip in place of every sub-batch's count / scan /
// write passes.  The pointers are DEVICE memory, the rows of query q at q * out_stride.
struct SortSpec {
  uint32_t column;
  uint32_t ascending, nulls_first;
  uint32_t out_stride;
  uint32_t *d_docs;
  uint64_t *d_values;
  uint8_t *d_has_value;
  uint32_t *d_counts;
  // sort_prepare: the slices per query, the key slots per lane the largest k needs; the column has a presence table
  uint32_t n_slices = 1, words_per_slice = 0, kpl = 1;
  bool optional = false;
};
// Aggregations (tq_agg.cpp): the aggregation launch of tq_agg.hip in place of every sub-batch's passes, behind one launch
// that initialises the whole batch's records and bucket rows.  d_stats / d_buckets are DEVICE memory, the record of
// query q at q, its row at q * bucket_stride.
struct AggSpec {
  uint32_t column;
  uint32_t value_type;          // TQ_VALUE_*
  tq_agg_hist_plan_t plan;      // n_buckets == 0: no histogram (none asked for, or no value can be in bounds)
  double interval, offset;
  uint32_t bucket_stride;
  tq_agg_stats_t *d_stats;
  uint32_t *d_buckets;
  uint32_t n_slices = 1, words_per_slice = 0;  // agg_prepare: as for a sort
  bool optional = false;
  // tq_agg_sub_batch*: a record of the metric column per bucket, at q * bucket_stride like the rows (null: no metric)
  const tq_agg_metric_request *metric = nullptr;
  tq_agg_bucket_stats_t *d_bucket_stats = nullptr;
  bool metric_optional = false;  // agg_prepare
  // tq_agg_terms_batch* (tq_agg_terms.cpp): in place of stats and histogram, the terms request (null: none) with its plan;
  // the record of query q at d_terms + q, its output rows at q * terms_stride; the count rows are the segment's scratch
  const tq_agg_terms_request *terms = nullptr;
  tq_agg_terms_plan_t terms_plan{};
  tq_agg_terms_t *d_terms = nullptr;
  uint64_t *d_term_keys = nullptr;
  uint32_t *d_term_counts = nullptr;
  uint32_t terms_stride = 0;
  // tq_agg_terms_sub_batch* (tq_agg_terms_sub.cpp): `terms` (a copy of the request's terms part) with a record of a metric
  // column per key and, maybe, an order by one metric of it; the survivors' records at q * terms_stride like the rows; the
  // count and record rows are the segment's scratch.  metric_optional as above
  const tq_agg_terms_sub_request *terms_sub = nullptr;
  tq_agg_bucket_stats_t *d_term_stats = nullptr;
  uint32_t terms_n_queries = 0;  // agg_terms_sub_prepare: the batch's queries
  // tq_agg_range_batch* (tq_agg_range.cpp): in place of the histogram, the range request (null: none) with its plan's buckets
  // (plan.n_buckets of them; nothing else of `plan`, interval and offset is read); counts at d_buckets, with `metric` the
  // records at d_bucket_stats, as for a histogram.  d_range_starts: agg_range_prepare's upload of the buckets' starts
  const tq_agg_range_request *range = nullptr;
  std::vector<tq_agg_range_bucket_t> range_plan;
  const uint64_t *d_range_starts = nullptr;
  // tq_agg_terms_hist_batch* (tq_agg_terms_hist.cpp): `terms` (the request's terms part) with a histogram of a second column
  // H per key — the request's hist part, its plan in `plan`, value_type / interval / offset as for a histogram; the
  // survivors' rows at d_buckets, row (q, j) at (q * terms_stride + j) * bucket_stride; the grid and totals rows are the
  // segment's scratch (terms_n_queries as above).  metric_optional: H has a presence table
  const tq_agg_terms_hist_request *terms_hist = nullptr;
  uint32_t terms_hist_cells = 0;  // n_keys x (n_buckets + 1)
};
// One call of the doc-set route: who consumes the match words of its sub-batches, and where the results go.
// kRows: CSR rows of ascending doc ids, `scored` with every doc's score beside it; kCount (host outputs): the count pass
// and out_starts alone, no doc is written (tq_count_batch); kSort / kAgg (device outputs): their spec.
enum class DocsetConsumer { kRows, kCount, kSort, kAgg };
struct DocsetCall {
  const char *fn;  // the entry point's name, for messages
  DocsetConsumer consumer;
  bool scored = false;
  bool device_out;  // the outputs are device buffers and the work is only enqueued, on hip_stream (null: the segment's)
  void *hip_stream = nullptr;
  uint32_t *out_docs = nullptr;  // kRows / kCount
  float *out_scores = nullptr;
  uint64_t out_cap = 0, *out_starts = nullptr;
  SortSpec *sort = nullptr;  // kSort
  AggSpec *agg = nullptr;    // kAgg
  // tq_count_batch hands over a sub-array of its n_caller queries: query qi of this call is the caller's caller_q[qi];
  // sloppy phrases are named, and their overflow words indexed, by that
  const uint32_t *caller_q = nullptr;
  uint32_t n_caller = 0;
  explicit DocsetCall(const char *name, DocsetConsumer c = DocsetConsumer::kRows)
      : fn(name), consumer(c), device_out(c == DocsetConsumer::kSort || c == DocsetConsumer::kAgg) {}
};
int docset_batch(tq_segment *s, const tq_query *queries, uint32_t n_queries, const DocsetCall &call);
// Consecutive whole queries whose lists without a bitmap, tree results and sloppy-phrase results fit the scratch together.
struct DocsetSubBatch {
  uint32_t q0 = 0, q1 = 0;
  size_t wg0 = 0, wg1 = 0;  // its part of the scatter work list
  uint32_t t0 = 0, t1 = 0;  // ... and of the tree records (tq_docset_tree.hip)
  uint32_t s0 = 0, s1 = 0;  // ... and of the sloppy phrases' records (tq_phrase_slop.hip)
  bool any_phrase = false;  // some tree of its queries has a phrase atom
  uint32_t n_temp = 0;      // its slots of the scratch
  bool score_blocks = false;  // some scoring list of its queries is reached by the block search
};
struct DocsetCut {
  std::vector<DocsetSubBatch> subs;
  std::vector<uint4> wgs;  // the scatter work list, sub-batch after sub-batch
  uint32_t max_sub_temp = 0, max_sub_n = 0;  // the most slots / queries of one sub-batch
};
// Cuts the batch (host arithmetic alone; checked on the CPU by tools/planbench/plan_check.cpp).  A sub-batch holds at
// most max_sub_queries queries and — unless it is a single query — max_temp slots.  In: every narrow dqs[].dense[m] the
// list's term handle; tree_q / slop_qi the ascending queries whose one list is the result of tqs[] / slop_qs[] in the
// same order; sqs empty or one per query.  Out: narrow dense[m] and part_start are SLOTS of their sub-batch's scratch.
void cut_docset_subs(const tq_segment *s, std::vector<TqkDocsetQuery> &dqs, const std::vector<TqkScoreQuery> &sqs,
                     const std::vector<uint32_t> &tree_q, std::vector<TqdTreeQuery> &tqs, const std::vector<uint32_t> &slop_qi,
                     std::vector<TqdSlopQuery> &slop_qs, uint32_t max_temp, uint32_t max_sub_queries, DocsetCut &cut);
// the scatter work list of one list without a bitmap: one entry (handle, first block, slot, 0) per four blocks
inline void push_scatter_work(std::vector<uint4> &wgs, const tq_segment *s, uint32_t handle, uint32_t slot) {
  for (uint32_t j = 0; j < s->terms[handle].n_blocks; j += 4u) wgs.push_back(make_uint4(handle, j, slot, 0u));
}
// ---- tq_sort.cpp / tq_agg.cpp as consumers of a doc-set call.  *_prepare, from the size-and-upload stage (the batch's
// scratch is idle, d_qmatches sized): the launch geometry into the spec, the consumer's buffers, uploads and zeroes on st.
// *_launch, per sub-batch behind its match bits: p is the sub-batch's filled TqkDocsetParams, q0 its first query.
uint32_t pick_slices(const tq_segment *s, int forced, uint32_t step_words, uint32_t max_sub_n, uint32_t n_words);
int sort_prepare(tq_segment *s, SortSpec &spec, const tq_query *queries, uint32_t n_queries, uint32_t max_sub_n, uint32_t n_words, hipStream_t st);
int sort_launch(tq_segment *s, const SortSpec &spec, const TqkDocsetParams &p, uint32_t q0, hipStream_t st);
int agg_prepare(tq_segment *s, AggSpec &spec, uint32_t n_queries, uint32_t max_sub_n, uint32_t n_words, hipStream_t st);
int agg_launch(tq_segment *s, const AggSpec &spec, const TqkDocsetParams &p, uint32_t q0, hipStream_t st);
// behind the last sub-batch's agg_launch, once: a terms aggregation's selection (anything else: nothing)
int agg_finish(tq_segment *s, const AggSpec &spec, uint32_t n_queries, hipStream_t st);
// tq_agg_terms.cpp: what the three do for a spec with `terms`
int agg_terms_prepare(tq_segment *s, AggSpec &spec, uint32_t n_queries, hipStream_t st);
int agg_terms_launch(tq_segment *s, const AggSpec &spec, const TqkDocsetParams &p, uint32_t q0, hipStream_t st);
int agg_terms_finish(tq_segment *s, const AggSpec &spec, uint32_t n_queries, hipStream_t st);
// the plan and the checks of a terms call under `fn`; max_order: the last order the call serves
int agg_terms_plan_checked(const char *fn, const tq_column_info_t &info, const tq_agg_terms_request &req, uint32_t max_order,
                           tq_agg_terms_plan_t *out);
int agg_terms_check_call(tq_segment *s, const char *fn, const tq_agg_terms_request *req, uint32_t max_order, const void *keys,
                         const void *counts, uint32_t out_stride, tq_agg_terms_plan_t *plan);
// tq_agg_range.cpp: for a spec with `range` — the starts' upload in front of agg_prepare's own work (the records and rows
// are a histogram's), and the launch; nothing follows the last sub-batch
int agg_range_prepare(tq_segment *s, AggSpec &spec, hipStream_t st);
int agg_range_launch(tq_segment *s, const AggSpec &spec, const TqkAggParams &a, uint32_t q0, hipStream_t st);  // a: agg_launch's
// tq_agg.cpp: the host-output variant of a checked call with rows of spec.plan.n_buckets entries (locked; spec without outputs)
int agg_host_run(tq_segment *s, const char *fn, const tq_query *queries, uint32_t n_queries, AggSpec &spec, tq_agg_stats_t *out_stats,
                 uint32_t *out_buckets, tq_agg_bucket_stats_t *out_bucket_stats, uint32_t bucket_stride);
// tq_agg_terms_sub.cpp: what the three do for a spec with `terms_sub`
int agg_terms_sub_prepare(tq_segment *s, AggSpec &spec, uint32_t n_queries, hipStream_t st);
int agg_terms_sub_launch(tq_segment *s, const AggSpec &spec, const TqkDocsetParams &p, uint32_t q0, hipStream_t st);
int agg_terms_sub_finish(tq_segment *s, const AggSpec &spec, uint32_t n_queries, hipStream_t st);
// tq_agg_terms_hist.cpp: what the three do for a spec with `terms_hist`
int agg_terms_hist_prepare(tq_segment *s, AggSpec &spec, uint32_t n_queries, hipStream_t st);
int agg_terms_hist_launch(tq_segment *s, const AggSpec &spec, const TqkDocsetParams &p, uint32_t q0, hipStream_t st);
int agg_terms_hist_finish(tq_segment *s, const AggSpec &spec, uint32_t n_queries, hipStream_t st);
// tq_agg.cpp: tq_agg_histogram_plan under `fn`
int agg_histogram_plan_checked(const char *fn, const tq_column_info_t &info, const tq_agg_request &req, tq_agg_hist_plan_t *out);
// A phrase or nested boolean query as plan_tree_query takes it for a doc set (option "docset_trees"): unit weights
// whatever the caller's are (doc sets score nothing; weights may be NULL), and a TQ_MODE_PHRASE query as the tree "one
// Must clause holding one phrase atom" with the caller's phrase_offsets.  scored (option "docset_score_trees"): the
// caller's weights (not NULL) are kept, a TQ_MODE_PHRASE query's weights[0] on every term of its atom.
struct TreeView {
  tq_query q;
  uint8_t occurs[TQ_MAX_TERMS], clause_of[TQ_MAX_TERMS], atom_of[TQ_MAX_TERMS], nested_occurs[TQ_MAX_TERMS];
  float weights[TQ_MAX_TERMS];
};
void docset_tree_view(const tq_query &q, TreeView &v, bool scored = false);  // (q.n_terms <= TQ_MAX_TERMS)
// ---- tq_phrase_slop.cpp: TQ_MODE_PHRASE with slop > 0
// A sloppy phrase as the tree planner takes it: the one-atom tree of docset_tree_view with the terms — and their offsets
// — in COST order (doc freq ascending, ties in phrase order), the order the reference's Intersection walks the lists in.
struct SlopView {
  TreeView v;
  tq_term_handle terms[TQ_MAX_TERMS];
  uint32_t offsets[TQ_MAX_TERMS];
};
// Validates query qi (slop != 0) and builds its view: TQ_ERR_INVALID a slop outside TQ_MODE_PHRASE, a malformed phrase,
// TQ_TERM_ALL or a term set in it; TQ_ERR_UNSUPPORTED slop > TQ_MAX_SLOP, more than 8 terms, a term of a field != 0.
// scored: weights[0] is kept (finite), else unit weights.
int slop_view(const tq_segment *s, const tq_query &q, uint32_t qi, const char *fn, SlopView &out, bool scored);
// The view's descriptor (plan_tree_query places the lists; n_terms 0: an absent term, nothing matches).  result_bitmap:
// the launch writes match bits that are read back (doc sets, counts).  qbytes: the HBM MODEL of the header, += .
int plan_slop_query(tq_segment *s, const tq_query &view, uint32_t qi, uint32_t slop, TqdSlopQuery &sq, uint64_t &qbytes, bool result_bitmap);
// TQ_ERR_UNSUPPORTED naming the first query with a non-zero overflow word, or TQ_OK
int slop_overflow_verdict(const char *fn, const uint32_t *over, uint32_t n_queries);
// ... over the words the last batch left on the device, read back (the batch is over); no sloppy phrase in it: TQ_OK
int slop_overflow_readback(tq_segment *s, const char *fn);
int slop_overflow_fail(const char *fn, uint32_t qi, uint32_t docs);
// ---- the planners
int build_group_chunks(Group &g, bool or_windows, PlanScratch &ps, bool boolean_group = false);
int build_share_plan(tq_segment *s, Group &g, PlanScratch &ps);
// resident: the wavefronts the launch keeps on the chip (its grid before the cap by the task count); 0 = not known
int build_ashare_plan(tq_segment *s, Group &g, PlanScratch &ps, bool boolean = false, uint32_t resident = 0);
int build_dense_plan(tq_segment *s, Group &g, PlanScratch &ps, uint32_t cus);
int plan_bool_query(tq_segment *s, const tq_query &q, uint32_t qi, TqdQuery &dq, uint64_t &qbytes,
                    uint32_t &n_tiles, uint32_t &tile_cost, uint32_t &n_thr_rows, bool exhaustive);
bool bool_query_is_tree(const tq_query &q);
int plan_tree_query(tq_segment *s, const tq_query &q, uint32_t qi, TqdTreeQuery &tq, uint64_t &qbytes, uint64_t table_base);
// ---- tq_search.cpp
int resolve_opts(const tq_segment *s, const tq_search_opts *o, CallOpts &co);
void update_table_span(tq_segment *s);
// the probe tables one nested boolean query needs (tq_tree.hip / tq_docset_tree.hip reach EVERY list through a bitmap,
// a phrase term's positions from the bitmap's rank); *built: some table is new (the tables' address span moved)
// flat_too: a flat TQ_MODE_BOOL query as well (one that names a term set: it takes the tree kernel)
int build_tree_query_probe_tables(tq_segment *s, const tq_query &q, bool *built, bool flat_too = false);
int fail_tree_tables(const tq_segment *s, uint32_t qi);  // "use_dense" off, or the tables outside one 32 GB span: TQ_ERR_UNSUPPORTED
int search_batch_impl(tq_segment *s, const tq_query *queries, uint32_t n_queries, uint32_t out_stride,
                      float *d_out_scores, uint32_t *d_out_docs, uint32_t *d_out_counts, void *hip_stream,
                      const CallOpts &co, uint32_t *d_out_segment_ords = nullptr, uint32_t segment_ord = 0);
// (a sloppy phrase over the carry cap: TQ_ERR_UNSUPPORTED naming the first such query, the rows written — or, under
// CallOpts::defer_slop_verdict, TQ_OK with the overflow words in tq_segment::slop_over_host)
int search_batch_host(tq_segment *s, const tq_query *queries, uint32_t n_queries, uint32_t out_stride,
                      float *out_scores, uint32_t *out_docs, uint32_t *out_counts, const CallOpts &co);
// The same in two halves (the submit queue: the next coalesced batch is planned and enqueued while this one runs):
// _begin plans and enqueues the batch on the segment's stream (caller holds the segment lock) — the merge kernels write
// scores | docs | counts into the slot's pinned host buffer — and records the slot's event; _end waits for that event
// (no lock needed) and leaves the rows readable at out.p, out.p + o_docs, out.p + o_counts.
struct HostBatchSlot {
  PinnedBuf out;
  size_t o_slop_over = 0;  // the batch's overflow words behind the rows (read when any_slop)
  bool any_slop = false;
  hipEvent_t done = nullptr, done_blocking = nullptr;  // the batch's last kernel: waited for spinning / asleep
  bool blocking = false;                               // ... which of the two this batch recorded
  size_t o_docs = 0, o_counts = 0;
  uint32_t n = 0, stride = 0;
};
int search_batch_host_begin(tq_segment *s, const tq_query *queries, uint32_t n_queries, uint32_t out_stride,
                            const CallOpts &co, HostBatchSlot &slot);
int search_batch_host_end(tq_segment *s, HostBatchSlot &slot);

}  // namespace tqi
