// tq_launch.h — kernel parameter blocks and launch entry points (tq_*.hip <-> tq_api.cpp)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tq_device.h"

// Output locations of a scan launch.  Kept in device memory behind ONE kernel-argument pointer:
// they are touched once per (chunk, query), and as kernel arguments they would pin 8 SGPRs of a
// kernel that is already spilling scalar registers.
struct TqkSinks {
  uint64_t *partials;                 // partial top-k lists, KPL*64 keys each
  unsigned long long *match_counter;  // docs scored by the whole launch
  uint32_t *query_matches;            // per query of the BATCH (through out_index): docs scored
  const uint32_t *out_index;          // launch-group query -> batch query
};

struct TqkScanParams {
  TqdSegment seg;
  const TqdTerm *terms;
  const TqdQuery *queries;      // the launch group's queries, contiguous
  const uint32_t *tile_starts;  // n_queries + 1, non-decreasing
  // one record per chunk, IN LAUNCH ORDER: {first tile, end tile, query of the first tile, chunk
  // id} — one 16-byte scalar load where a permutation lookup, two neighbouring starts and a
  // binary search over the queries' tile ranges (~14 dependent loads) used to be
  const uint4 *chunk_recs;
  const float *caches;          // n_caches x 256
  const TqkSinks *sinks;        // where results go (read at flush time only)
  uint32_t *thr_slots;          // [n_thr_rows][TQD_THR_SLOTS] shared thresholds (pruned mode)
  uint32_t n_queries;
  uint32_t total_tiles;
  uint32_t n_chunks;
  uint32_t exhaustive;  // 1: score every match; 0: block-max pruning allowed
  uint32_t use_dense;   // 0: ignore the dense-list bitmaps (always seek + decode)
  uint32_t max_terms;   // largest n_terms among the launch's queries
  uint32_t or_windows;  // OR: 1 = window-parallel kernel, 0 = candidate-driven kernel
  uint32_t debug;       // TQ_DEBUG ablation bits (profiling only; results are wrong when set)
  uint32_t all_dense;   // AND: every non-leader list of every query of the launch has a bitmap
  uint32_t boolean;     // union kernel: queries carry roles / clauses / min_should (TQ_MODE_BOOL)
  uint32_t small_k;     // every query of the launch has k <= 16
  float bound_slack;    // >= 1: widens block-max bounds when the BM25 statistics are not the segment's own
};

// shared-union launch: a persistent grid of single-wave workgroups pulling tasks
struct TqkShareParams {
  TqdSegment seg;
  const TqdTerm *terms;
  const TqdQuery *queries;      // the launch group's queries (part_start / n_parts count list ENTRIES)
  const float *caches;
  const TqdLead *leads;
  const uint4 *tasks;           // {term handle, first block, n_blocks | n_leads << 16 | cache << 24, first lead}
  const TqkSinks *sinks;
  uint32_t *thr_slots;          // hashed score slots per query (as the other pruned kernels use)
  uint32_t *thr_val;            // [n_queries] current lower bound of each query's k-th best score
  uint32_t *task_counter;       // next task to hand out (zeroed per batch)
  const uint8_t *table_base;    // TqdLead::dense_off / tf8_off count 8-byte units from here
  uint64_t *stage;              // [grid][TQD_US_GROUP][capl] per-wave staging lists
  uint64_t *lists;              // per-query result lists (query q: entries part_start .. + n_parts)
  uint32_t *list_count;         // [n_queries] entries written so far
  uint32_t task_begin, n_tasks; // this launch hands out tasks [task_begin, n_tasks)
  uint32_t n_queries;
  uint32_t grid;
  uint32_t debug;
  float bound_slack;
};

// shared-intersection launch (tq_ashare.hip): a persistent grid of single-wave workgroups pulling tasks
struct TqkAShareParams {
  TqdSegment seg;
  const TqdTerm *terms;
  const TqdQuery *queries;      // boolean leads: the launch group's queries (part_start / n_parts count list ENTRIES)
  const TqdAQuery *aqueries;    // intersections: their compact records ...
  const TqdQuery *xqueries;     // ... and the full records of those with three and more lists (TqdAQuery::ext)
  const float *caches;
  const TqdALead *leads;
  const uint4 *tasks;           // {leader term handle, first block, n_blocks | n_leads << 16 | cache << 24, first lead}
  const uint2 *qlists;          // boolean leads: [query][TQD_AS_MAX_TERMS] = {bitmap, tf bytes} of its lists (as dense_off / tf8_off)
  const TqkSinks *sinks;
  uint32_t *thr_slots;          // hashed score slots per query (as the other pruned kernels use)
  uint32_t *thr_val;            // [n_queries] current lower bound of each query's k-th best score
  uint32_t *task_counter;       // [n_queues] next task of each queue to hand out (zeroed per batch)
  const uint8_t *table_base;    // TqdALead::dense_off / tf8_off count 8-byte units from here
  uint64_t *stage;              // [grid][TQD_AS_GROUP][capl] per-wave staging lists
  uint64_t *lists;              // per-query result lists (query q: entries part_start .. + n_parts)
  uint32_t *list_count;         // [n_queries] entries written so far
  uint32_t task_begin, n_tasks; // this launch hands out tasks [task_begin, n_tasks)
  uint32_t n_queries;
  uint32_t grid;
  uint32_t debug;
  uint32_t boolean;             // the leads are (TQ_MODE_BOOL query, leading list) pairs
  uint32_t rdir_lists;          // ... and some entry of qlists is a range directory (the instantiation that knows them)
  float bound_slack;
  uint32_t n_queues;            // task queues of this launch (1, or 8 = one per XCD)
  uint32_t bound_mode;          // TQ_AS_BOUND bits: where list 1's range maxima replace its weight as the bound
};

// exhaustive pure unions, doc-major (tq_xunion.hip): a persistent grid of 16-wave workgroups; a
// workgroup builds the BM25 term scores of EVERY (list, weight) pair of the group for a tile of 128
// docs in LDS, then each of its waves evaluates its share of the group's queries against that tile
constexpr uint32_t TQK_XU_TILE = 128;         // docs per tile (two per lane)
constexpr uint32_t TQK_XU_MAX_ROWS = 256;     // rows of the tile: up to 255 distinct (list, weight) pairs + the all-zero padding row
constexpr uint32_t TQK_XU_MAX_QUERIES = 8192; // queries of a group
#ifndef TQK_XU_WAVES_N
#define TQK_XU_WAVES_N 16
#endif
constexpr uint32_t TQK_XU_WAVES = TQK_XU_WAVES_N;
struct TqkDenseRow {  // one posting list of the group.  Rows with a bitmap come first.
  const uint2 *dense;         // bitmap + rank directory (TqdTermHead::dense), or null
  const uint8_t *tf8;         // byte-wide tfs by posting index (with `dense`, or with `flat_docs`); null = every tf is 1
  const uint32_t *flat_docs;  // lists without a bitmap: the decoded doc ids (doc_freq entries)
  uint32_t handle;            // the list's term record (saturated tf bytes are read from the packed stream)
  uint32_t doc_freq;
  float w;                    // the row holds w * tf/(tf+norm): a list used at two weights is two rows
  uint32_t pad;
};
struct TqkDenseQuery {  // 16 bytes, loaded one query per lane
  uint32_t rows_lo, rows_hi;  // row of list t in byte t (lists in score-sum order); beyond n_terms: row n_rows (all zero)
  uint32_t nt_k;              // n_terms | k << 8
  uint32_t thr_row;           // first row of the query's threshold slots (64 for k <= 16, else 256)
};
struct TqkDenseParams {
  TqdSegment seg;
  const TqdTerm *terms;
  const TqkDenseRow *rows;
  const TqkDenseQuery *queries;
  const float *cache;           // Bm25Weight.cache of the group (256 floats)
  const TqkSinks *sinks;
  uint32_t *thr_slots;
  uint32_t *thr_val;            // [n_queries]
  uint32_t *list_count;         // [n_queries]
  uint32_t *task_counter;
  uint64_t *stage;              // [grid][n_queries][capl] staging lists private to a workgroup
  uint64_t *lists;              // [n_queries][list_stride] result lists
  uint32_t n_rows, n_bitmap_rows;
  uint32_t n_queries;
  uint32_t max_terms;           // the most lists a query of the launch has
  uint32_t n_tasks, tiles_per_task;
  uint32_t list_stride;
  uint32_t grid;
  uint32_t debug;
};

struct TqkMergeParams {
  const TqdQuery *queries;    // (tqk_launch_merge_lists with `compact`: TqdAQuery records)
  const uint64_t *partials;
  const uint32_t *out_index;  // query -> output row (null = identity)
  float *out_scores;
  uint32_t *out_docs;
  uint32_t *out_counts;
  uint32_t n_queries;
  uint32_t out_stride;
  // two-level merge (queries with thousands of partial lists: a small batch cut into short tiles): `pre_slices` > 0 =
  // a first launch of n_queries x pre_slices wavefronts reduces slice s of every query's lists — lists [s * per,
  // (s + 1) * per), per = tqk_merge_slice_lists(n_parts, pre_slices) — into the slice's FIRST list, in place; the
  // final launch then reads one list per slice.  Queries with fewer than TQK_MERGE_PRE_MIN lists are left alone.
  uint32_t pre_slices;
  // an index of one segment: the rows are merge_top_k's already, this is its column of segment ordinals ([query][out_stride],
  // write_topk_rows in tq_common.hpp); null = no such column
  uint32_t *out_segment_ords;
  uint32_t segment_ord;
};
constexpr uint32_t TQK_MERGE_PRE_MIN = 96;
inline __host__ __device__ uint32_t tqk_merge_slice_lists(uint32_t n_parts, uint32_t pre_slices) {
  return (pre_slices == 0u || n_parts < TQK_MERGE_PRE_MIN) ? 1u : (n_parts + pre_slices - 1u) / pre_slices;
}

struct TqkSegMergeParams {
  const float *scores;          // [segment][query][stride]
  const uint32_t *docs;
  const uint32_t *counts;       // [segment][query]
  const uint32_t *segment_ords; // [segment] or null
  float *out_scores;            // [query][limit]
  uint32_t *out_segment_ords;
  uint32_t *out_docs;
  uint32_t *out_counts;
  uint32_t n_segments, n_queries, stride, offset, limit;
};

// ---- nested boolean queries over bitmaps (tq_tree.hip): a BooleanQuery whose clauses are terms or BooleanQuerys of
// terms.  Terms of a clause are contiguous; clauses in score-sum order (Must clauses cheapest first, then Should,
// then MustNot); inside a clause Must terms first.  Occurs: TQD_ROLE_* (= enum tq_occur).
constexpr uint32_t TQK_TREE_TILE_WORDS = 4096;  // bitmap words (131 072 docs) per (query, tile) wavefront
constexpr uint32_t TQK_TREE_MAX_TERMS = 16;
constexpr uint32_t TQK_TREE_PHRASE_TERMS = 8;  // terms of a phrase inside a boolean query (one position cursor each, in registers)
struct TqdTreeQuery {
  uint32_t n_terms, n_clauses;   // 0 / 0: the planner found the query empty
  uint32_t k, cache_idx;
  uint32_t part_start;           // first partial top-k list (one per tile); tq_docset_tree.hip: the query's result slot
  uint32_t top_has_must;         // the query has Must clauses (else: the union of its Should clauses)
  uint32_t top_need;             // Should clauses that have to match: minimum_number_should_match, at least 1 without a Must clause
  uint32_t has_phrase;           // some atom is a PhraseQuery (atom_end bit 1): the bitmap expression is a superset, every doc is re-checked
  uint32_t dense_off[TQK_TREE_MAX_TERMS];    // bitmap + rank directory / byte-wide tfs of the term's list, as offsets
  uint32_t tf8_off[TQK_TREE_MAX_TERMS];      // from TqkTreeParams::table_base in 8-byte units
  uint32_t weight_bits[TQK_TREE_MAX_TERMS];  // (float) idf * (1 + k1) * boost
  uint32_t handle[TQK_TREE_MAX_TERMS];       // term handle (saturated tf bytes read the packed value)
  uint32_t inner[TQK_TREE_MAX_TERMS];        // occur of the term's ATOM inside its clause (an atom = a run of terms that
                                             // must all be present: one term, or a nested intersection of terms)
  uint32_t atom_end[TQK_TREE_MAX_TERMS];     // bit 0: the term is the last of its atom; bit 1 (on every term of the atom): the atom is
                                             // a PhraseQuery of <= TQK_TREE_PHRASE_TERMS terms (weight_bits = the phrase's weight);
                                             // bit 2 (on every term of the atom): the atom is a UNION of its terms (present where
                                             // any of them is, scoring the present ones) instead of a conjunction;
                                             // bit 3: a CONST-SCORE leaf (a term set): present where its bit is, scoring
                                             // weight_bits as given — neither rank nor tf is read (tf8_off = dense_off)
                                             // bits 4..6: the FIELD of the list (multi-field segments; 0 = the primary field)
  uint32_t dir_off[TQK_TREE_MAX_TERMS];      // phrase terms: position directory of the list (TqdTerm::pos_dir layout), 8-byte units
  uint32_t phrase_off[TQK_TREE_MAX_TERMS];   // phrase terms: max_offset - term_offset (phrase_scorer.rs:372-385)
  uint32_t outer[TQK_TREE_MAX_TERMS];        // per clause: its occur in the query
  uint32_t inner_need[TQK_TREE_MAX_TERMS];   // per clause: Should terms that have to be present
  uint32_t first_term[TQK_TREE_MAX_TERMS + 1];  // per clause: its terms are [first_term[c], first_term[c + 1])
};
struct TqkTreeParams {
  TqdSegment seg;
  const TqdTerm *terms;
  const TqdTreeQuery *queries;
  const float *caches;
  const TqkSinks *sinks;
  const uint8_t *table_base;
  uint32_t n_queries, n_words;
  uint32_t any_phrase;  // some query of the launch has a phrase atom (selects the kernel instantiation)
};
hipError_t tqk_launch_tree(const TqkTreeParams &p, int kpl, hipStream_t st);
// The same trees over the lists of SEVERAL fields (tq_fields.cpp): tree_fields_kernel, tq_tree_fields.hip.  The field
// of list t rides in bits 4..6 of TqdTreeQuery::atom_end[t] (the other kernels that read the record test single bits
// below them); list t of field f scores under caches[(cache_idx + f) * 256 + fn[f][doc]] — fn[f] null: the constant
// id — so a query's cache is F consecutive rows.  fn[0] = the segment's own fieldnorms.  These launch parameters alone
// know about fields: TqdSegment stays as it is.
constexpr uint32_t TQK_MAX_FIELDS = 8;
struct TqkTreeFieldsParams {
  TqkTreeParams base;
  const uint8_t *fn[TQK_MAX_FIELDS];
};
hipError_t tqk_launch_tree_fields(const TqkTreeFieldsParams &p, int kpl, hipStream_t st);
uint32_t tqk_tree_tiles(uint32_t n_words);
// ---- the exact match bits of such trees for doc sets (tq_docset_tree.hip): query q's alive matching docs as bits
// [part_start * words_per_list, + n_words) of the doc-set batch's scratch, every word stored once; no scores
struct TqkDocsetTreeParams {
  TqdSegment seg;
  const TqdTerm *terms;
  const TqdTreeQuery *queries;  // [n_queries] as plan_tree_query leaves them (k / cache_idx / weight_bits are not read)
  const uint8_t *table_base;
  uint32_t *bits;               // the scratch's result bitmaps: words_per_list 32-bit words each
  uint32_t n_queries, n_words, words_per_list;
  uint32_t any_phrase;          // some query of the launch has a phrase atom (selects the kernel instantiation)
};
hipError_t tqk_launch_docset_tree(const TqkDocsetTreeParams &p, hipStream_t st);

// ---- sloppy phrases (tq_phrase_slop.hip): TQ_MODE_PHRASE with slop > 0 over the lists' bitmaps, in the tree route's
// geometry (tiles of TQK_TREE_TILE_WORDS words, one partial top-k list per (query, tile), tqk_tree_tiles).  Lists in
// COST order (doc freq ascending, ties in phrase order): the order the reference walks them in.
constexpr uint32_t TQK_SLOP_MAX_TERMS = TQK_TREE_PHRASE_TERMS;
constexpr uint32_t TQK_SLOP_CARRY_CAP = 32;  // = TQ_SLOP_CARRY_CAP (tantivy_amd.h; asserted in tq_phrase_slop.cpp)
struct TqdSlopQuery {                        // 192 bytes
  uint32_t n_terms;                          // 2..8; 0: the planner found the query empty (an absent term)
  uint32_t k, cache_idx;
  uint32_t part_start;                       // first partial top-k list (one per tile); doc sets: the query's result slot
  uint32_t slop;                             // 1..255
  uint32_t weight_bits;                      // (float) the phrase's weight: (1 + k1) * boost * sum of idfs
  uint32_t out_q;                            // query of the BATCH: its overflow word
  uint32_t pad_;
  uint32_t dense_off[TQK_SLOP_MAX_TERMS];    // bitmap + rank directory / byte-wide tfs / position directory of the list,
  uint32_t tf8_off[TQK_SLOP_MAX_TERMS];      // as offsets from TqkPhraseSlopParams::table_base in 8-byte units
  uint32_t dir_off[TQK_SLOP_MAX_TERMS];
  uint32_t phrase_off[TQK_SLOP_MAX_TERMS];   // max_offset - term_offset (phrase_scorer.rs:372-385)
  uint32_t handle[TQK_SLOP_MAX_TERMS];       // term handle (positions; saturated tf bytes read the packed value)
};
static_assert(sizeof(TqdSlopQuery) == 192, "TqdSlopQuery is uploaded as raw bytes");
struct TqkPhraseSlopParams {
  TqdSegment seg;
  const TqdTerm *terms;
  const TqdSlopQuery *queries;
  const float *caches;          // scoring launch
  const TqkSinks *sinks;        // scoring launch
  const uint8_t *table_base;
  uint32_t *overflow;           // [batch queries] candidate docs whose carried list went over the cap (zeroed by the caller)
  uint32_t *bits;               // bits launch: the scratch's result bitmaps, words_per_list 32-bit words each
  uint32_t n_queries, n_words, words_per_list;
  uint32_t any_pair;            // some query has 2 lists or is empty / some has 3 or more: one launch per instantiation,
  uint32_t any_carry;           // so that a 2-list query never pays for the carried lists
};
hipError_t tqk_launch_phrase_slop(const TqkPhraseSlopParams &p, int kpl, hipStream_t st);
hipError_t tqk_launch_phrase_slop_bits(const TqkPhraseSlopParams &p, hipStream_t st);

// ---- ALL-BASED queries (tq_all.hip): a flat query whose AllQuery clauses (TQ_TERM_ALL) make every doc a candidate
// (tq_all.cpp).  Lists: the Should lists in score-sum order (clause by clause, query order), then the MustNot lists.
constexpr uint32_t TQK_ALL_TILE_WORDS = 2048;  // bitmap words (65 536 docs) per (query, tile) wavefront
struct TqdAllQuery {              // 288 bytes
  uint32_t n_lists, n_should;     // lists [0, n_should): Should; [n_should, n_lists): MustNot (bits only)
  uint32_t clause_end;            // bit t: Should list t is the last of its clause (a clause counts once and sums first)
  uint32_t min_should;            // 0: every doc; m >= 1: the docs that hold at least m Should clauses (m <= 15)
  uint32_t base_bits;             // (float) what every doc of the set scores before its Should clauses: 1.0, or the sole All's boost
  uint32_t k, cache_idx;
  uint32_t part_start;            // first partial top-k list (one per scanned tile)
  uint32_t n_tiles;               // tiles the query scans: the segment's, or — no list, no alive bitset — the ceil(k / 65 536) first
  uint32_t extra_matches;         // docs of the tiles it does not scan (they all match)
  uint32_t pad_[2];
  uint32_t dense_off[TQD_MAX_TERMS];    // bitmap + rank directory / byte-wide tfs of the list, as offsets from
  uint32_t tf8_off[TQD_MAX_TERMS];      // TqkAllParams::table_base in 8-byte units
  uint32_t weight_bits[TQD_MAX_TERMS];  // (float) idf * (1 + k1) * boost
  uint32_t handle[TQD_MAX_TERMS];       // term handle (saturated tf bytes read the packed value)
};
struct TqkAllParams {
  TqdSegment seg;
  const TqdTerm *terms;
  const TqdAllQuery *queries;
  const float *caches;
  const TqkSinks *sinks;
  const uint8_t *table_base;
  uint32_t n_queries, n_words, max_tiles;  // max_tiles: the most tiles a query of the launch scans
};
hipError_t tqk_launch_all(const TqkAllParams &p, int kpl, hipStream_t st);
uint32_t tqk_all_tiles(uint32_t n_words);

hipError_t tqk_launch_and(const TqkScanParams &p, int kpl, bool use_dpp, hipStream_t st);
hipError_t tqk_launch_or(const TqkScanParams &p, int kpl, bool use_dpp, hipStream_t st);
hipError_t tqk_launch_phrase(const TqkScanParams &p, int kpl, bool use_dpp, hipStream_t st);
hipError_t tqk_launch_merge(const TqkMergeParams &p, int kpl, hipStream_t st);
hipError_t tqk_launch_share(const TqkShareParams &p, int kpl, hipStream_t st);
// merge of the shared-union launch's per-query lists (m.partials = lists, list_count per query)
// the words a batch zeroes before its kernels (match counters, threshold slots, the shared launches' per-query words):
// ONE launch instead of a fill per buffer (five fills and their gaps were 30 us of a 1.1 ms headline step, 15 of a
// 140 us one-query call)
constexpr int TQK_ZERO_MAX = 8;
struct TqkZeroParams {
  uint32_t *ptr[TQK_ZERO_MAX];  // 4-byte aligned
  uint32_t words[TQK_ZERO_MAX];
  uint32_t n;
};
// tf classes of a column list into TqdSegment::doccls (slot < TQD_CLS_SLOTS; the words zeroed at allocation)
hipError_t tqk_launch_doccls_set(uint64_t *cls, const uint32_t *docs, const uint32_t *tfs, uint32_t n, uint32_t slot,
                                 uint32_t max_doc, hipStream_t st);
hipError_t tqk_launch_zero(const TqkZeroParams &p, hipStream_t st);
// signature bits (TQD_SIG_SHIFT + bits[i]) of n lists, given by their own records, into the doc matrix: one launch
// ... and, where tabs[i] is not null, the list's range directory (rdir_lookup, tq_common.hpp: tabs[i] = (max_doc >>
// shifts[i]) + 2 directory slots padded to a multiple of four, then dfs[i] entries; nothing needs zeroing); bits[i] =
// 0xFFFFFFFF: no signature bit for list i; mat may be null.  cache (256 floats: the segment's own Bm25 cache) not null:
// lmax_out[i] (zeroed) gets the list's largest tf/(tf + norm) as build_rmax rounds it
hipError_t tqk_launch_docsig_batch(const TqdSegment &seg, const TqdTerm *const *selfs, const uint32_t *bits, uint32_t n,
                                   uint64_t *mat, uint32_t *const *tabs, const uint32_t *shifts, const uint32_t *dfs,
                                   const float *cache, uint32_t *lmax_out, bool use_dpp, hipStream_t st);
// ... from a decoded list (docs / tfs: n postings, ascending)
hipError_t tqk_launch_rdir_fill(const uint32_t *docs, const uint32_t *tfs, uint32_t n, uint32_t max_doc, uint32_t *dir,
                                uint32_t S, hipStream_t st);
// (compact: m.queries points at TqdAQuery records — the shared intersections' group)
hipError_t tqk_launch_merge_lists(const TqkMergeParams &m, const uint32_t *list_count, int kpl, bool compact,
                                  hipStream_t st);
uint32_t tqk_share_capl(int kpl);  // staging entries per lead slot
// ---- Count collector over bitmaps (tq_count.hip)
#define TQK_COUNT_MUST 0u
#define TQK_COUNT_NOT 1u
#define TQK_COUNT_SHOULD 2u
#define TQK_COUNT_HAS_MUST 1u     // flags: the doc set is the intersection of the Must clauses (else: the union of the Should lists)
#define TQK_COUNT_NEED_SHOULD 2u  // flags: ... and at least one Should list (minimum_number_should_match = 1)
struct TqkCountQuery {            // 152 bytes
  uint32_t n_terms;               // lists: Must clauses first (a clause = a union of lists), then MustNot, then Should
  uint32_t kinds;                 // 2 bits per list: TQK_COUNT_*
  uint32_t clause_end;            // bit m: list m is the last of its Must clause
  uint32_t flags;
  uint32_t narrow;                // bit m: list m's bitmap is a plain array of 32-bit words (a list without a
  uint32_t pad_;                  // bitmap of its own, scattered into the batch's scratch: count_scatter_kernel)
  const uint2 *dense[TQD_MAX_TERMS];  // the lists' bitmaps: {32 doc bits, postings before the word}
};
struct TqkCountParams {
  const TqkCountQuery *queries;
  const uint8_t *alive;  // AliveBitSet bits or null
  uint32_t *out_counts;  // [n_queries], zeroed by the caller
  uint32_t n_queries, n_words;
};
hipError_t tqk_launch_count_bitmaps(const TqkCountParams &p, hipStream_t st);
// the docs of lists without a bitmap as bits: wgs[i] = {term handle, first block, slot, -}: 4 blocks per workgroup
hipError_t tqk_launch_count_scatter(const TqdSegment &seg, const TqdTerm *terms, const uint4 *wgs, uint32_t n_wgs,
                                    uint32_t *bits, uint32_t words_per_list, hipStream_t st);
uint32_t tqk_count_tile_words();
// ---- term sets (tq_termset.hip): the bitmap + rank directory of the OR of many lists into `tab` (n_words + 1 entries,
// zeroed by the caller).  d_members: the n_members bitmaps of the members that have one; d_items: {member's term handle,
// first block} per four blocks of the members that have none; scan_scratch: tqk_termset_scratch_words(n_words) words —
// afterwards its word ceil(n_words / tqk_termset_scan_tile()) (at least 1) holds the set's doc count
hipError_t tqk_launch_termset_build(const TqdSegment &seg, const TqdTerm *terms, const uint2 *const *d_members, uint32_t n_members,
                                    const uint2 *d_items, uint32_t n_items, uint2 *tab, uint32_t n_words, uint32_t *scan_scratch,
                                    hipStream_t st);
uint32_t tqk_termset_scan_tile();
uint32_t tqk_termset_scratch_words(uint32_t n_words);
// ... its rank stage alone, over a table of n_words + 1 entries whose .x words are written (bits at and past max_doc in the
// last word are cleared first): tab[w].y = docs before word w, tab[n_words] = {0, docs}, scan_scratch as above
hipError_t tqk_launch_bitmap_rank(uint2 *tab, uint32_t n_words, uint32_t max_doc, uint32_t *scan_scratch, hipStream_t st);
// ---- fast-field ranges (tq_range.hip): a u64_based column-values payload in HBM (tq_column.cpp) against a value range
#define TQK_COL_BITPACKED 0u
#define TQK_COL_LINEAR 1u
#define TQK_COL_BLOCKWISE 2u
struct TqkColBlock {   // 32 bytes: one block of 512 rows of a BlockwiseLinear column
  uint64_t slope, intercept;  // its Line
  uint64_t data_off;          // byte offset of its bit-packed diffs in the payload (a multiple of 64)
  uint32_t bit_width, pad_;
};
struct TqkColumn {
  const uint32_t *payload;    // the codec's payload from its first byte, 256-byte aligned, 16 zero bytes behind it
  const TqkColBlock *blocks;  // BlockwiseLinear: ceil(num_rows / 512) records
  const uint2 *present;       // TQ_CARD_OPTIONAL: {32 presence bits, rows before the word} per 32 docs; null: row = doc
  uint64_t slope, intercept;  // Linear: its Line
  uint32_t codec, num_bits;   // num_bits: Bitpacked / Linear (BlockwiseLinear: per block)
  uint32_t num_rows, max_doc;
};
// tab[w].x = the docs of word w whose packed value n lies in [lo, hi] (both inclusive; Linear: n is the value itself),
// every word of the table written; the rank stage follows
hipError_t tqk_launch_range_fill(const TqkColumn &col, uint64_t lo, uint64_t hi, uint2 *tab, uint32_t n_words, hipStream_t st);
// out[i] = min + gcd * n of row first_row + i (Linear: n), i < n; the caller has checked first_row + n <= num_rows
hipError_t tqk_launch_column_decode(const TqkColumn &col, uint64_t min_value, uint64_t gcd, uint32_t first_row, uint32_t n,
                                    uint64_t *out, hipStream_t st);
// ---- full doc sets over bitmaps (tq_docset.hip): the expression of TqkCountQuery with the result bits kept
struct TqkDocsetQuery {           // 152 bytes
  uint32_t n_terms;               // lists: Must clauses first (a clause = a union of lists), then MustNot, then Should
  uint32_t kinds;                 // 2 bits per list: TQK_COUNT_*
  uint32_t clause_end;            // bit m: list m is the last of its Must clause
  uint32_t should_end;            // bit m: list m is the last of its Should clause (a clause counts once)
  uint32_t narrow;                // bit m: list m's bitmap is a plain array of 32-bit words (the batch's scratch)
  uint32_t min_should;            // 0: the Must clauses alone; m >= 1: ... and at least m of the Should clauses (m <= 15);
                                  // a query without Must clauses is the union of its Should clauses: 1.
                                  // The empty doc set: no lists and min_should = 1
  const uint2 *dense[TQD_MAX_TERMS];  // the lists' bitmaps: {32 doc bits, postings before the word}
};
struct TqkDocsetParams {
  const TqkDocsetQuery *queries;  // [n_queries] (one sub-batch)
  const uint8_t *alive;           // AliveBitSet bits or null
  uint32_t *tile_counts;          // [n_queries][n_tiles] docs per (query, tile): written by the count pass
  uint64_t *tile_offs;            // ... their exclusive prefix sum, from *base_in: written by the scan
  uint64_t *partials;             // [ceil(n_queries * n_tiles / tqk_docset_scan_tile())] scan scratch
  const uint64_t *base_in;        // docs of the sub-batches before this one (null: 0)
  uint64_t *out_starts;           // [n_queries + 1] the sub-batch's part of the CSR row starts
  uint32_t *query_sizes;          // [n_queries] docs per query
  unsigned long long *total_out;  // docs so far, this sub-batch included
  uint32_t *out_docs;             // the write pass stores no doc at or past out_cap
  uint64_t out_cap;
  uint32_t n_queries, n_tiles, n_words, max_doc;
  uint32_t stage_min_docs;        // write pass: a tile with at least this many docs goes through an LDS slab
};
hipError_t tqk_launch_docset_count(const TqkDocsetParams &p, hipStream_t st);
hipError_t tqk_launch_docset_scan(const TqkDocsetParams &p, hipStream_t st);
hipError_t tqk_launch_docset_write(const TqkDocsetParams &p, hipStream_t st);
uint32_t tqk_docset_tile_words();
uint32_t tqk_docset_scan_tile();
// ---- sort by fast field (tq_sort.hip): the top k of a doc set under a u64 column's order (tq_search_sorted_batch*).
// The selection launch: workgroup = (query, slice of the bitmap words), query fastest; with n_slices == 1 it writes the
// rows, else a sorted partial list per (query, slice) that the merge launch, one wavefront per query, reduces.
struct TqkSortParams {
  TqkDocsetParams ds;          // queries (one sub-batch), alive, n_queries, n_words, max_doc: what docset_word reads
  TqkColumn col;               // the sort column
  uint64_t min_value, gcd;     // value = min + gcd * packed (Linear: the packed value itself)
  const uint32_t *ks;          // [n_queries] every query's k, 1..TQ_MAX_K
  uint64_t *partials;          // [n_queries][n_slices][2][kpl * 64]: the slices' lists, hi words then lo words (n_slices > 1)
  uint2 *slice_counts;         // [n_queries][n_slices] {matches, matches with a value} (n_slices > 1)
  uint32_t *out_docs;          // rows of the sub-batch's first query on: [n_queries][out_stride]
  uint64_t *out_values;
  uint8_t *out_has_value;
  uint32_t *out_counts;        // [n_queries]
  uint32_t *query_sizes;       // [n_queries] alive matches per query
  unsigned long long *totals;  // [3] += matches, matches with a value, row entries written (zeroed by the caller)
  uint32_t n_slices, words_per_slice;
  uint32_t out_stride;
  uint32_t ascending;          // TQ_SORT_ASC
  uint32_t nulls_first;        // TQ_NULLS_FIRST
};
// kpl: key slots per lane, 1 / 4 / 16 (k <= 64 / 256 / 1024 for every query of the launch)
hipError_t tqk_launch_sort_select(const TqkSortParams &p, int kpl, hipStream_t st);
hipError_t tqk_launch_sort_merge(const TqkSortParams &p, int kpl, hipStream_t st);
uint32_t tqk_sort_step_words();  // bitmap words a selection workgroup takes per step
// ---- aggregations over a fast field (tq_agg.hip): stats and a histogram of a u64 column over a doc set (tq_agg_batch*).
// One launch: workgroup = (query, slice of the bitmap words), query fastest; every workgroup adds its part to the query's
// record (and bucket row) with vector atomics, so the records and rows are initialised in front of it (tqk_launch_agg_init).
struct TqkAggStats {  // = tq_agg_stats_t, 64 bytes
  unsigned long long matches, count, min_value, max_value, sum_lo, sum_hi, in_bounds, out_of_range;
};
struct TqkAggParams {
  TqkDocsetParams ds;          // queries (one sub-batch), alive, n_queries, n_words, max_doc: what docset_word reads
  TqkColumn col;               // the aggregated column
  uint64_t min_value, gcd;     // value = min + gcd * packed (Linear: the packed value itself)
  TqkAggStats *stats;          // records of the sub-batch's first query on: [n_queries]
  uint32_t *buckets;           // rows of the sub-batch's first query on: [n_queries][bucket_stride] (histogram)
  uint32_t *query_sizes;       // [n_queries] += alive matches per query (zeroed by the caller)
  unsigned long long *totals;  // [2] += matches, matches with a value (zeroed by the caller)
  double interval, offset;     // pos = floor((val - offset) / interval)
  double bounds_min, bounds_max;  // the effective bounds (tq_agg_hist_plan_t): val is counted when min <= val <= max
  int64_t base_pos;            // bucket of a row's entry 0
  uint32_t n_buckets;          // entries of a row the launch may write (0 = no histogram)
  uint32_t bucket_stride;
  uint32_t lds_buckets;        // n_buckets <= this: a workgroup-private table in LDS, flushed at the end; above: the row
  uint32_t value_type;         // TQ_VALUE_*: how a u64-space value becomes the f64 the histogram buckets
  uint32_t n_slices, words_per_slice;
};
hipError_t tqk_launch_agg_init(TqkAggStats *stats, uint32_t *buckets, uint32_t n_queries, uint32_t n_buckets,
                               uint32_t bucket_stride, hipStream_t st);
hipError_t tqk_launch_agg(const TqkAggParams &p, hipStream_t st);
uint32_t tqk_agg_step_words();   // bitmap words an aggregation workgroup takes per step
uint32_t tqk_agg_lds_buckets();  // the LDS table's compile-time capacity in buckets
// ---- sub-aggregations (tq_agg_sub.hip): the launch above with a record of a METRIC column B per bucket of the histogram
// (tq_agg_sub_batch*).  The records, like the rows, are added to with vector atomics: tqk_launch_agg_sub_init in front.
struct TqkAggBucketStats {  // = tq_agg_bucket_stats_t, 40 bytes
  unsigned long long count, min_value, max_value, sum_lo, sum_hi;
};
struct TqkAggSubParams {
  TqkAggParams a;              // the bucket column A and everything tqk_launch_agg takes (n_buckets >= 1); a.totals is [5]:
                               // += matches, matches with a value in A, -, bucketed docs with a value in B, bucketed docs
  TqkColumn col_b;             // the metric column
  uint64_t min_value_b, gcd_b;
  TqkAggBucketStats *bucket_stats;  // records of the sub-batch's first query on: [n_queries][a.bucket_stride]
  uint32_t value_type_b;       // TQ_VALUE_F64: no sum
};
hipError_t tqk_launch_agg_sub_init(TqkAggBucketStats *bucket_stats, uint32_t n_queries, uint32_t n_buckets, uint32_t bucket_stride,
                                   hipStream_t st);
hipError_t tqk_launch_agg_sub(const TqkAggSubParams &p, hipStream_t st);
// the LDS tables' compile-time capacities in buckets: out[0] the small instantiation's, out[1] the large one's
void tqk_agg_sub_lds_capacities(uint32_t out[2]);
// ---- range aggregation (tq_agg_range.hip): doc counts per range of column A over a doc set and, with a metric, a record of
// column B per range (tq_agg_range_batch*).  The ranges are the host plan's buckets; the launch takes their STARTS in the
// column's u64 space.  tqk_launch_agg_init (and, with a metric, tqk_launch_agg_sub_init) in front, as for the histogram.
struct TqkAggRangeParams {
  TqkAggSubParams s;       // everything tqk_launch_agg_sub takes; of s.a the histogram's interval / offset / bounds / base_pos
                           // are not read, 1 <= s.a.n_buckets <= 1 024; without a metric col_b and bucket_stats are not read
                           // and s.a.totals is [3]
  const uint64_t *starts;  // [s.a.n_buckets] non-decreasing, starts[0] == 0: a value's bucket is the last start <= it
};
hipError_t tqk_launch_agg_range(const TqkAggRangeParams &p, bool metric, hipStream_t st);
// the record table's compile-time capacities in buckets (with a metric): out[0] the small instantiation's, out[1] the large one's
void tqk_agg_range_lds_capacities(uint32_t out[2]);
// ---- terms aggregation (tq_agg_terms.hip): doc counts per key of a column over a doc set, then the top segment_size
// entries per query (tq_agg_terms_batch*).  tqk_launch_agg_terms_init in front; one count launch per sub-batch adds to the
// records and to the per-query scratch rows with vector atomics; one select launch behind the last of them writes the output
// rows and the rest of the records.
struct TqkAggTerms {  // = tq_agg_terms_t, 40 bytes
  unsigned long long matches, count, sum_other_doc_count;
  uint32_t distinct, n_returned, doc_count_error_upper_bound, out_of_range;
};
struct TqkAggTermsParams {
  TqkDocsetParams ds;          // queries (one sub-batch), alive, n_queries, n_words, max_doc: what docset_word reads
  TqkColumn col;               // the aggregated column
  uint64_t min_value, gcd;     // key index = (value - min) / gcd: the packed value (Linear: computed)
  TqkAggTerms *records;        // records of the sub-batch's first query on: [n_queries]
  uint32_t *rows;              // scratch rows of the sub-batch's first query on: [n_queries][n_keys]
  uint32_t *query_sizes;       // [n_queries] += alive matches per query (zeroed by the caller)
  unsigned long long *totals;  // [5] += matches, matches with a value, -, entries returned (the select launch), - (zeroed by the caller)
  uint32_t n_keys;             // entries of a scratch row, <= TQ_AGG_MAX_BUCKETS
  uint32_t lds_buckets;        // n_keys <= this: a workgroup-private table in LDS, flushed at the end; above: the row
  uint32_t n_slices, words_per_slice;
};
struct TqkAggTermsSelectParams {
  TqkAggTerms *records;        // [n_queries] of the whole batch
  const uint32_t *rows;        // [n_queries][n_keys]
  uint64_t *out_keys;          // [n_queries][out_stride]: entries [0, n_returned) of a row are written
  uint32_t *out_counts;        // the same
  unsigned long long *totals;  // [3] += n_returned
  uint64_t min_value, gcd;     // key = min + gcd * index
  uint32_t n_queries, n_keys, out_stride;
  uint32_t segment_size;       // 1 .. tqk_agg_terms_max_size()
  uint32_t order;              // TQ_TERMS_ORDER_*
};
hipError_t tqk_launch_agg_terms_init(TqkAggTerms *records, uint32_t *rows, uint32_t n_queries, uint32_t n_keys, hipStream_t st);
hipError_t tqk_launch_agg_terms_count(const TqkAggTermsParams &p, hipStream_t st);
hipError_t tqk_launch_agg_terms_select(const TqkAggTermsSelectParams &p, hipStream_t st);
void tqk_agg_terms_lds_capacities(uint32_t out[2]);  // the count kernel's two LDS tables, in keys: small, large
uint32_t tqk_agg_terms_max_size();                   // the largest segment_size
// ---- terms aggregation with a metric (tq_agg_terms_sub.hip): the launches above with a record of a METRIC column B per key
// and a selection that may order by one metric of it (tq_agg_terms_sub_batch*).  The scratch is per query a count row and a
// record row of n_keys entries each; the select launch also writes the survivors' records.
struct TqkAggTermsSubParams {
  TqkAggTermsParams t;         // the key column A and everything the count launch takes; t.totals is [6]: += matches, matches
                               // with a value in A, -, entries returned (the select launch), counted docs with a value in B,
                               // counted docs
  TqkColumn col_b;             // the metric column
  uint64_t min_value_b, gcd_b;
  TqkAggBucketStats *stats;    // scratch records of the sub-batch's first query on: [n_queries][t.n_keys]
  uint32_t value_type_b;       // TQ_VALUE_F64: no sum
};
struct TqkAggTermsSubSelectParams {
  TqkAggTermsSelectParams s;       // s.order: TQ_TERMS_* up to TQ_TERMS_METRIC_ASC
  const TqkAggBucketStats *stats;  // [n_queries][s.n_keys]
  TqkAggBucketStats *out_stats;    // [n_queries][s.out_stride]: entries [0, n_returned) of a row are written
  uint32_t value_type_b;           // TQ_VALUE_* of B
  uint32_t metric;                 // tq_terms_metric, read under the two metric orders
};
hipError_t tqk_launch_agg_terms_sub_init(TqkAggTerms *records, uint32_t *rows, TqkAggBucketStats *stats, uint32_t n_queries,
                                         uint32_t n_keys, hipStream_t st);
hipError_t tqk_launch_agg_terms_sub_count(const TqkAggTermsSubParams &p, hipStream_t st);
hipError_t tqk_launch_agg_terms_sub_select(const TqkAggTermsSubSelectParams &p, hipStream_t st);
void tqk_agg_terms_sub_lds_capacities(uint32_t out[2]);  // the count kernel's two LDS tables, in keys: small, large
// ---- terms x histogram (tq_agg_terms_hist.hip): a histogram of a column H per key of a column T over a doc set
// (tq_agg_terms_hist_batch*).  The scratch is per query a GRID row of n_cells = n_keys x (n_buckets + 1) entries — key i's
// row at i x (n_buckets + 1), its last entry the docs outside the histogram — and a TOTALS row of n_keys entries.
// tqk_launch_agg_terms_hist_init in front; one count launch per sub-batch adds to the records and the grid rows with vector
// atomics; behind the last of them the row sums into the totals rows, tqk_launch_agg_terms_select over the totals rows, and
// the gather of the survivors' rows.
struct TqkAggTermsHistParams {
  TqkAggTermsParams t;         // the key column T and everything the terms count launch takes; t.rows: the GRID rows of the
                               // sub-batch's first query on, [n_queries][n_cells]; t.lds_buckets against n_cells; t.totals is
                               // [6]: += matches, matches with a value in T, -, entries returned (the select launch), counted
                               // docs with a value in H, counted docs
  TqkColumn col_h;             // the histogram column
  uint64_t min_value_h, gcd_h;
  double interval, offset;     // pos = floor((val - offset) / interval)
  double bounds_min, bounds_max;  // the effective bounds (tq_agg_hist_plan_t)
  int64_t base_pos;            // bucket of a key row's entry 0
  uint32_t n_buckets;          // a key's row has n_buckets + 1 entries
  uint32_t value_type_h;       // TQ_VALUE_*
};
struct TqkAggTermsHistFinishParams {
  const TqkAggTerms *records;  // [n_queries] of the whole batch (the gather reads n_returned)
  const uint32_t *grid;        // [n_queries][n_keys x (n_buckets + 1)]
  uint32_t *totals_rows;       // [n_queries][n_keys]: the row-sum launch writes every entry
  const uint64_t *out_keys;    // [n_queries][out_stride]: what the select launch wrote
  uint32_t *out_hist;          // [n_queries][out_stride][hist_stride]: entries [0, n_buckets) of rows [0, n_returned)
  uint64_t min_value, gcd;     // index = (key - min) / gcd
  uint32_t n_queries, n_keys, n_buckets;
  uint32_t out_stride, hist_stride;
  uint32_t width;              // min(segment_size, n_keys): the most entries a query returns
};
hipError_t tqk_launch_agg_terms_hist_init(TqkAggTerms *records, uint32_t *grid, uint32_t *totals_rows, uint32_t n_queries, uint32_t n_cells,
                                          uint32_t n_keys, hipStream_t st);
hipError_t tqk_launch_agg_terms_hist_count(const TqkAggTermsHistParams &p, hipStream_t st);
hipError_t tqk_launch_agg_terms_hist_rowsum(const TqkAggTermsHistFinishParams &p, hipStream_t st);
hipError_t tqk_launch_agg_terms_hist_gather(const TqkAggTermsHistFinishParams &p, hipStream_t st);
void tqk_agg_terms_hist_lds_capacities(uint32_t out[2]);  // the count kernel's two LDS tables, in cells: small, large
// ---- scores of full doc sets (tq_docset_score.hip): the pass behind the write pass of a tq_docset_scored_batch* call.
// How a scoring list answers "is doc d in the list, with which tf" (chosen by the host per list):
#define TQK_SCORE_BITMAP 0u  // tab = the list's bitmap + rank directory, aux = its byte-wide tfs (null: read the block)
#define TQK_SCORE_RDIR 1u    // tab = its range directory, aux = the directory's entries, shift = the directory's shift
#define TQK_SCORE_BLOCKS 2u  // seek_block + lookup_in_blocks over the packed list
#define TQK_SCORE_CONST 3u   // a term set (tq_termset.cpp): tab = its bitmap, present = the doc's bit, score = weight as given
struct TqkScoreQuery {             // 472 bytes: every non-MustNot list of the query, in the order its scores are summed
  uint32_t n_lists;                // 0: the query matches nothing
  uint32_t cache_idx;              // which 256-float Bm25Weight cache of the batch
  uint32_t access;                 // 2 bits per list: TQK_SCORE_*
  uint32_t clause_end;             // bit m: list m is the last of its clause (a clause = the sum of its present lists)
  uint32_t n_must_lists;           // lists [0, n_must_lists): the Must clauses, cheapest first (Intersection::score: first +
                                   // second + the sum of the others); behind them the Should clauses (req + opt, or the union)
  uint32_t all_base_bits;          // an ALL-BASED query (TQ_TERM_ALL clauses, tq_all.cpp): the float added LAST to the sum of the
                                   // present Should clauses — a doc that no list holds scores it; 0 = not such a query
  uint32_t handle[TQD_MAX_TERMS];  // term record (exact tfs of saturated entries, the block search)
  float weight[TQD_MAX_TERMS];
  uint32_t shift[TQD_MAX_TERMS];
  const void *tab[TQD_MAX_TERMS];
  const void *aux[TQD_MAX_TERMS];
};
struct TqkScoreParams {
  TqdSegment seg;
  const TqdTerm *terms;
  const TqkScoreQuery *queries;    // [n_queries] (one sub-batch)
  const float *caches;             // n_caches x 256
  const uint32_t *tile_counts;     // [n_queries][n_tiles] and their prefix sum: what the sub-batch's count pass and scan left
  const uint64_t *tile_offs;
  const uint32_t *out_docs;        // the rows the write pass has just stored
  float *out_scores;               // out_scores[i] = the score of out_docs[i]; nothing at or past out_cap
  uint64_t out_cap;
  uint32_t n_queries, n_tiles;
  uint32_t any_blocks;             // some list of the sub-batch is TQK_SCORE_BLOCKS (selects the instantiation with LDS)
};
hipError_t tqk_launch_docset_score(const TqkScoreParams &p, hipStream_t st);
// ... with scoring lists of SEVERAL fields (tq_fields.cpp): docset_score_fields_kernel, tq_docset_score_fields.hip.  The field of
// list m rides in bits 8..10 of TqkScoreQuery::shift[m] (zero on every list of a launch that takes the kernel above,
// whose range-directory lookup reads the whole word); norms as in TqkTreeFieldsParams.
struct TqkScoreFieldsParams {
  TqkScoreParams base;
  const uint8_t *fn[TQK_MAX_FIELDS];
};
hipError_t tqk_launch_docset_score_fields(const TqkScoreFieldsParams &p, hipStream_t st);
// ---- ... of phrases and nested boolean queries (tq_docset_tree_score.hip, option "docset_score_trees"): the pass behind the
// write pass over the sub-batch's TREE queries, whose rows the flat pass leaves alone.  Tree i of the launch is query
// query_of[i] of the sub-batch: that is where its tile_counts / tile_offs stand.
struct TqkDocsetTreeScoreParams {
  TqdSegment seg;
  const TqdTerm *terms;
  const TqdTreeQuery *queries;     // [n_queries] as plan_tree_query leaves them, cache_idx set (k / part_start are not read)
  const uint32_t *query_of;        // [n_queries] tree -> query of the sub-batch
  const float *caches;             // n_caches x 256: the blob the flat pass reads
  const uint8_t *table_base;
  const uint32_t *tile_counts;     // [sub-batch queries][n_tiles] and their prefix sum
  const uint64_t *tile_offs;
  const uint32_t *out_docs;        // the rows the write pass has just stored
  float *out_scores;               // out_scores[i] = the score of out_docs[i]; nothing at or past out_cap
  uint64_t out_cap;
  uint32_t n_queries, n_tiles;
  uint32_t any_phrase;             // some tree of the launch has a phrase atom (selects the instantiation with position cursors)
};
hipError_t tqk_launch_docset_tree_score(const TqkDocsetTreeScoreParams &p, hipStream_t st);
hipError_t tqk_launch_ashare(const TqkAShareParams &p, int kpl, hipStream_t st);
uint32_t tqk_ashare_waves_per_cu();  // resident wavefronts per CU the kernel is built for
uint32_t tqk_bshare_waves_per_cu();  // ... its boolean instantiation
hipError_t tqk_launch_xunion(const TqkDenseParams &p, int kpl, hipStream_t st);
// a list without a bitmap as plain arrays: doc ids and min(tf, 255) per posting
hipError_t tqk_launch_flat_list(const TqdSegment &seg, const TqdTerm *terms, uint32_t handle,
                                uint32_t n_blocks, uint32_t *docs, uint8_t *tf8, hipStream_t st);
// the fieldnorm ids of a list's docs in posting order, 128 bytes per block (TermHost::lnorm_blob; needs a fieldnorm file)
hipError_t tqk_launch_lead_norms(const TqdSegment &seg, const TqdTerm *terms, uint32_t handle, uint32_t n_blocks,
                                 uint8_t *out, hipStream_t st);
// the doc-matrix words of a list's docs in posting order, 128 u64 per block (TermHost::lmat_blob)
hipError_t tqk_launch_lead_mat(const TqdSegment &seg, const TqdTerm *terms, uint32_t handle, uint32_t n_blocks,
                               uint64_t *out, hipStream_t st);
hipError_t tqk_launch_decode_list(const TqdSegment &seg, const TqdTerm *terms, uint32_t handle,
                                  uint32_t n_blocks, uint32_t *docs, uint32_t *tfs, bool use_dpp,
                                  hipStream_t st);
hipError_t tqk_launch_decode_positions(const TqdSegment &seg, const TqdTerm *terms,
                                       uint32_t handle, uint32_t *out, uint64_t n, hipStream_t st);
hipError_t tqk_launch_merge_segments(const TqkSegMergeParams &p, hipStream_t st);
// doc matrix (TqdSegment::docmat): fill with the fieldnorm ids / set one list's column
hipError_t tqk_launch_docmat_init(uint64_t *mat, const uint8_t *fieldnorm, uint32_t const_id,
                                  uint32_t max_doc, hipStream_t st);
hipError_t tqk_launch_docmat_set(uint64_t *mat, const uint32_t *docs, uint32_t n, uint32_t slot,
                                 uint32_t max_doc, hipStream_t st);
// term freqs of a decoded list as bytes (TqdTerm::tf8)
hipError_t tqk_launch_tf8_pack(const uint32_t *tfs, uint32_t n, uint8_t *out, hipStream_t st);


// ---- shared with tq_encode.hip: the C ABI's error slot and context checks live in tq_api.cpp
struct tq_ctx;
int tq_internal_fail(int code, const char *where, const char *what);
bool tq_internal_ctx_has_device(const tq_ctx *ctx, int device);
