/*
 * tantivy_amd_host.h — flat C entry points over the C++ host mirror (tantivy_amd/host/): the
 * Searcher / Query::weight / TopDocs surface of the reference (src/core/searcher.rs:180-238,
 * src/query/query.rs:128-160, src/collector/top_score_collector.rs:61-96) driving the device
 * through tantivy_amd.h.  Used by the Python tests and bench; a C++ application includes
 * tantivy_amd/host/searcher.hpp directly.
 */
#ifndef TANTIVY_AMD_HOST_H
#define TANTIVY_AMD_HOST_H
#include "tantivy_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct tqh_searcher tqh_searcher;

/* TermInfo (src/postings/term_info.rs:10-17) keyed by a caller-chosen term id; stands in for the
 * reference's TermDictionary, which stays with the caller (termdict untouched). */
typedef struct tqh_term_info {
  uint32_t term_id;
  uint32_t doc_freq;
  uint64_t postings_start, postings_end, positions_start, positions_end;
} tqh_term_info;

/* mode: the values of enum tq_mode (tantivy_amd.h) —
 *       TQ_MODE_AND (0) = BooleanQuery of Must term clauses, TQ_MODE_OR (1) = BooleanQuery of
 *       Should term clauses, TQ_MODE_PHRASE (2) = PhraseQuery (offsets 0..n unless phrase_offsets
 *       given; `slop` as PhraseQuery::set_slop: scoring calls count matches, Count and doc sets test
 *       existence, and the two verdicts differ as in the reference — tantivy_amd.h "Sloppy phrases",
 *       the overflow contract included), TQ_MODE_BOOL (3) = BooleanQuery with per-term occurs (0 Should, 1 Must,
 *       2 MustNot); terms sharing a clause_of value form one nested query: a union of its terms
 *       (`+a +(b OR c)`) or, with nested_occurs, a BooleanQuery with an occur per term
 *       (`+a +(+b -c)`: clause_of {0,1,1}, occurs {1,1,1}, nested_occurs {255,1,2}; 255 / NULL =
 *       Should).  A Must clause holding a nested query with a Must term is hoisted into its
 *       parent (boolean_weight.rs:308-431: same docs, same score terms); the other nestings of
 *       depth 2 — an intersection inside a union or under MustNot, nested MustNot / optional
 *       terms, a nested minimum_number_should_match (clause_min_should) — run on the device over
 *       the lists' bitmaps (TQ_KERNEL_TREE); deeper trees and phrases inside boolean queries are
 *       TQ_ERR_UNSUPPORTED and stay on tantivy's CPU scorer;
 *       min_should_match as BooleanQuery::set_minimum_number_should_match —
 *       plus TQH_MODE_TERM (4) = TermQuery.  Anything else: TQ_ERR_INVALID.
 *       terms[i] == TQ_TERM_ALL (every mode but TQ_MODE_PHRASE): the clause is an AllQuery (Query::all()), boosts[i] its
 *       BoostQuery factor; a query of that one term is the AllQuery itself, and a one-clause BooleanQuery of it ignores
 *       min_should_match (BooleanWeight::scorer, boolean_weight.rs:463-469).  Inside a nested query: TQ_ERR_UNSUPPORTED. */
#define TQH_MODE_TERM 4
typedef struct tqh_query {
  uint8_t mode;
  uint32_t n_terms;
  const uint32_t *terms;
  const uint32_t *phrase_offsets;
  const uint8_t *occurs;
  const uint8_t *clause_of;
  uint32_t min_should_match;
  uint32_t slop; /* TQ_MODE_PHRASE: PhraseQuery::set_slop (tantivy_amd.h "Sloppy phrases"); any other mode: 0.  Sits in what
                    was padding: sizeof(tqh_query) is unchanged, and callers must zero the struct */
  const float *boosts; /* per term: the TermQuery is wrapped in BoostQuery(boost) (boost_query.rs);
                          PHRASE: boosts[0] wraps the PhraseQuery; NULL = 1 */
  const uint8_t *nested_occurs; /* TQ_MODE_BOOL: occur of a term inside its clause_of group (read for
                                   groups of >= 2 terms); NULL = unions */
  const uint8_t *clause_min_should; /* TQ_MODE_BOOL: minimum_number_should_match of the nested query of a
                                       clause_of group, 16 entries indexed by the clause_of value; NULL = 0 */
  const uint8_t *atom_of; /* TQ_MODE_BOOL: terms of one clause_of group sharing an atom_of value are ONE member of the
                             nested query — an intersection of terms one level further down (`+a +((+b +c) d)`:
                             clause_of {0,1,1,1}, atom_of {0,1,1,2}, nested_occurs {-,0,0,0}); NULL = every term its own */
  /* Term sets (Query::term_set: TermSetQuery and every other AutomatonWeight query — the docs of the named terms OR-ed
   * into a bitset that scores the boost, tantivy_amd.h "term sets"): terms[i] == TQH_TERM_SET_BASE + j names set j, whose
   * term ids are set_terms[set_starts[j] .. set_starts[j + 1]); boosts[i] its BoostQuery factor = the score of every doc
   * of the set.  Every mode but TQ_MODE_PHRASE, as a query of its own or a direct clause; inside a nested query:
   * TQ_ERR_UNSUPPORTED.  Both NULL: no sets.  The sets are prepared per segment when the batch first runs and released
   * with the prepared batch. */
  const uint32_t *set_terms;
  const uint32_t *set_starts;
} tqh_query;
#define TQH_TERM_SET_BASE 0xFFFFFF00u

const char *tqh_last_error(void);
int tqh_searcher_new(tq_ctx *ctx, tqh_searcher **out);
void tqh_searcher_free(tqh_searcher *s);
/* SegmentReader for one field of one segment; segment_ord = order of addition. */
int tqh_searcher_add_segment(tqh_searcher *s, int device, uint32_t max_doc, uint8_t record_option,
                             const uint8_t *idx, size_t idx_len, const uint8_t *pos,
                             size_t pos_len, const uint8_t *fieldnorm, size_t fn_len,
                             const tqh_term_info *terms, uint32_t n_terms);
/* SegmentReader for n_fields fields of one segment over one doc-id space (tq_segment_upload_fields in tantivy_amd.h:
 * fields[f] = field f's sub-files, one record_option for all; field 0 is the primary field).  term_fields[i] = the
 * field of terms[i] (NULL: all of field 0); term ids share ONE uint32_t space over the fields, a term id belongs to one
 * field.  Queries name term ids as on a single-field segment: every term scores with its own field's fieldnorms and
 * the Bm25Weight cache under its own field's average fieldnorm (idf from its own doc_freq), a query that names a term
 * of a field != 0 runs as TQ_KERNEL_TREE, and a phrase over terms of different fields is TQ_ERR_INVALID (the
 * reference's PhraseQuery panics on it). */
int tqh_searcher_add_segment_fields(tqh_searcher *s, int device, uint32_t max_doc, uint8_t record_option,
                                    uint32_t n_fields, const tq_field_files *fields, const tqh_term_info *terms,
                                    const uint8_t *term_fields, uint32_t n_terms);
/* Bm25StatisticsProvider input for segments held by other ranks (src/query/bm25.rs:11-50):
 * their max_doc, total_num_tokens and per-term doc_freq are added to the local sums. */
int tqh_searcher_add_remote_stats(tqh_searcher *s, uint64_t max_doc, uint64_t total_num_tokens,
                                  const uint32_t *term_ids, const uint32_t *doc_freqs,
                                  uint32_t n_terms);
/* ... of multi-field segments: tokens[f] = their total_num_tokens of field f (the call above means field 0). */
int tqh_searcher_add_remote_stats_fields(tqh_searcher *s, uint64_t max_doc, const uint64_t *tokens, uint32_t n_fields,
                                         const uint32_t *term_ids, const uint32_t *doc_freqs, uint32_t n_terms);
/* Query::weight for every query of a batch (global BM25 statistics + executor choice). */
int tqh_prepare_batch(tqh_searcher *s, const tqh_query *queries, uint32_t n);
/* Query::weight of the NEXT batch while the current one executes on another thread (a second slot; thread-safe next to
 * the tqh_collect_* / tqh_search_* calls of the current batch), and the switch to it: tqh_commit_next is called by the
 * executing thread between two batches, after tqh_prepare_batch_next has returned. */
int tqh_prepare_batch_next(tqh_searcher *s, const tqh_query *queries, uint32_t n);
int tqh_commit_next(tqh_searcher *s);
/* Searcher::search of the prepared batch with TopDocs::with_limit(limit).and_offset(offset):
 * outputs [n][limit], (score desc, segment_ord asc, doc asc). */
int tqh_search_prepared(tqh_searcher *s, uint32_t offset, uint32_t limit, float *scores,
                        uint32_t *segment_ords, uint32_t *docs, uint32_t *counts);
/* Searcher::search called from n_threads host threads at once, one query per call — the reference's
 * own call pattern (src/core/searcher.rs:180-238): thread t takes queries t, t + n_threads, ...;
 * every call is Query::weight + one tq_search_one per segment (the calls of concurrent threads ride
 * in shared launches) + merge_fruits.  Outputs [n][limit] as tqh_search_prepared; latency_ms[q] =
 * wall time of query q's call (may be NULL); *wall_ms = the whole run (may be NULL). */
int tqh_search_concurrent(tqh_searcher *s, const tqh_query *queries, uint32_t n, uint32_t offset,
                          uint32_t limit, uint32_t n_threads, float *scores, uint32_t *segment_ords,
                          uint32_t *docs, uint32_t *counts, float *latency_ms, double *wall_ms);
/* Searcher::search(&query, &Count) of the prepared batch (src/collector/count_collector.rs:39-80):
 * counts[q] = alive matching docs summed over the segments. */
int tqh_count_prepared(tqh_searcher *s, uint64_t *counts);
/* Searcher::search(&query, &DocSetCollector) of the prepared batch (src/collector/docset_collector.rs:26-57): query q
 * owns the pairs (out_segment_ords[i], out_docs[i]), i in out_starts[q] .. out_starts[q+1], the alive matching docs of
 * every segment (tq_docset_batch) ordered by (segment_ord, doc) — the DocAddresses merge_fruits unions.  out_starts has
 * n + 1 entries and is filled whenever the queries are valid; if out_starts[n] exceeds out_cap the call fails, has
 * written no pair, and the caller retries with buffers of out_starts[n] entries.  Flat queries only (tantivy_amd.h,
 * "doc sets"): a phrase or a nested query fails the batch as unsupported, unless the option "docset_trees" is set on
 * every segment. */
int tqh_docset_prepared(tqh_searcher *s, uint32_t *out_segment_ords, uint32_t *out_docs, uint64_t out_cap,
                        uint64_t *out_starts);
/* The same for a collector that needs scores (Weight::for_each: TopDocs::tweak_score / custom_score, a MultiCollector
 * with a scoring child): out_scores[i] = the BM25 score of pair i under the searcher's index-wide statistics
 * (tq_docset_scored_batch on every segment).  Same rows, same capacity protocol; one out_cap covers the three arrays.
 * A phrase or a nested query fails the batch as unsupported unless the option "docset_score_trees" (tantivy_amd.h, "doc
 * sets with scores") is set on every segment; "docset_trees" does not concern this call. */
int tqh_docset_scored_prepared(tqh_searcher *s, uint32_t *out_segment_ords, uint32_t *out_docs, float *out_scores,
                               uint64_t out_cap, uint64_t *out_starts);
/* Collector::collect_segment of the prepared batch on one segment: [n][k] sorted. */
int tqh_collect_segment_prepared(tqh_searcher *s, uint32_t segment_ord, uint32_t k, float *scores,
                                 uint32_t *docs, uint32_t *counts);
/* Same with DEVICE output pointers, enqueued on hip_stream without a host sync. */
int tqh_collect_segment_prepared_device(tqh_searcher *s, uint32_t segment_ord, uint32_t k,
                                        float *d_scores, uint32_t *d_docs, uint32_t *d_counts,
                                        void *hip_stream);
/* Searcher::search of the prepared batch with TopDocs::with_limit(k) on the device as ONE call (src/core/searcher.rs:
 * 180-238: collect_segment on every segment, then merge_fruits): everything is enqueued on hip_stream, the host never
 * waits.  out_* ([n][k] x 3, [n]): device memory, or pinned host memory mapped into the device.  Rows as
 * tqh_search_prepared(offset 0, limit k) leaves them.
 *   one segment       its merge kernels write the four arrays themselves (tq_search_batch_device_rows): no merge_top_k
 *                     launch, the slabs are not touched and may be NULL
 *   several segments  segment s collects into part s of the slabs (d_slab_scores / d_slab_docs: [S][n][k],
 *                     d_slab_counts: [S][n], device memory on the segments' one device), then ONE tq_merge_topk_device
 *                     launch; HIP events around it feed tqh_exchange_ms */
int tqh_search_prepared_device(tqh_searcher *s, uint32_t k, float *out_scores, uint32_t *out_segment_ords,
                               uint32_t *out_docs, uint32_t *out_counts, float *d_slab_scores,
                               uint32_t *d_slab_docs, uint32_t *d_slab_counts, void *hip_stream);
/* *ms = mean GPU time of the merge_top_k launches of the last (<= 16) tqh_search_prepared_device calls since the
 * previous tqh_exchange_ms (waits for them to finish); 0.0 when none ran, as with one segment. */
int tqh_exchange_ms(tqh_searcher *s, float *ms);
/* Bm25Weight::for_terms(...).boost_by(boost): weight + 256-entry tf cache — of ONE field: the statistics passed in are
 * that field's (total_num_tokens of the field).  It knows no Searcher.  A caller that builds raw tq_query records
 * against a multi-field segment calls it once per field with that field's token count and lays the F caches end to
 * end (tq_query.tf_cache = F x 256 floats, row f = field f); one 256-float cache there is too short. */
int tqh_bm25_for_terms(const uint64_t *term_doc_freqs, uint32_t n_terms, uint64_t total_num_docs,
                       uint64_t total_num_tokens, float boost, float *weight_out,
                       float *cache_out);
tq_segment *tqh_segment_raw(tqh_searcher *s, uint32_t segment_ord);
uint32_t tqh_term_handle(tqh_searcher *s, uint32_t segment_ord, uint32_t term_id);

/* ---- term dictionary values ----
 * replaces: TermInfoStore::{open, get} and TermInfoStoreWriter (src/termdict/fst_termdict/
 * term_info_store.rs:130-163, :166-290).  The FST (term bytes -> ordinal) stays with tantivy-fst;
 * everything after the ordinal is here, so a query batch crosses the boundary as ordinals.
 * tqh_term_dictionary_values: where the store sits inside a field's term dictionary file
 * (TermDictionary::open, termdict.rs:123-140 inside the wrapper of src/termdict/mod.rs:82-98:
 * fst | store | u64 store_len | u32 fst version | u32 dictionary type). */
typedef struct tqh_term_info_store tqh_term_info_store;
int tqh_term_dictionary_values(const uint8_t *file, size_t len, uint64_t *store_off,
                               uint64_t *store_len);
int tqh_term_info_store_open(const uint8_t *bytes, size_t len, tqh_term_info_store **out);
void tqh_term_info_store_free(tqh_term_info_store *s);
uint64_t tqh_term_info_store_num_terms(const tqh_term_info_store *s);
/* out[i] = TermInfo of term_ords[i] (term_id = the ordinal) */
int tqh_term_info_store_get(const tqh_term_info_store *s, const uint64_t *term_ords, uint32_t n,
                            tqh_term_info *out);
/* TermInfoStoreWriter::{write_term_info*, serialize} over infos in ordinal order; *out_len =
 * bytes needed (also when the buffer was too small). */
int tqh_term_info_store_write(const tqh_term_info *infos, uint32_t n, uint8_t *out,
                              uint64_t out_cap, uint64_t *out_len);
/* tqh_searcher_add_segment with the segment's TermInfoStore instead of a TermInfo array: term
 * ids are term ordinals and TermInfos are decoded on first use. */
int tqh_searcher_add_segment_with_store(tqh_searcher *s, int device, uint32_t max_doc,
                                        uint8_t record_option, const uint8_t *idx, size_t idx_len,
                                        const uint8_t *pos, size_t pos_len,
                                        const uint8_t *fieldnorm, size_t fn_len,
                                        const uint8_t *store, size_t store_len);

/* The same for sub-files that are resident on `device` (tq_segment_upload_device): device
 * pointers; total_num_tokens = the value of the .idx sub-file's 8-byte header. */
int tqh_searcher_add_segment_device_with_store(tqh_searcher *s, int device, uint32_t max_doc,
                                               uint8_t record_option, const uint8_t *d_idx,
                                               size_t idx_len, const uint8_t *d_pos, size_t pos_len,
                                               const uint8_t *d_fieldnorm, size_t fn_len,
                                               uint64_t total_num_tokens, const uint8_t *store,
                                               size_t store_len);

#ifdef __cplusplus
}
#endif
#endif
