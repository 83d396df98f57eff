/*
 * tantivy_amd.h — C ABI of the MI355X-native query-execution path for tantivy.
 *
 * This is the drop-in boundary: everything below
 * `Weight::for_each_pruning` / `Collector::collect_segment` — posting-list decode, AND / OR /
 * exact-phrase evaluation, BM25, per-segment top-k and the cross-segment merge — runs on the
 * GPU behind these entry points.  Plain pointers and sizes only; callable from Rust through a
 * thin `extern "C"` crate (binding shown in INTEGRATION.md), from C++ (tantivy_amd/host/) and
 * from Python ctypes (tantivy_amd/binding.py).
 *
 * Ownership: inputs are borrowed for the duration of the call (segment bytes are copied to HBM
 * by tq_segment_upload); outputs are caller-allocated; handles are opaque and freed explicitly.
 * Every function returns TQ_OK (0) or an error code; tq_last_error() gives the message of the
 * last failure on the calling thread.  Nothing here panics or throws across the boundary.
 *
 * Thread-safety: every entry point that takes a tq_segment locks it for the duration of the call
 * (term table, planner scratch and staging buffers are per segment), so concurrent callers on one
 * segment are serialised, never undefined; different segments run concurrently — tantivy's own
 * "one task per segment" executor model (src/core/executor.rs:44-106).  Many threads each issuing
 * single queries should use tq_search_one / tq_submit + tq_wait below: their queries are coalesced
 * into batched launches instead of queueing up one launch each.
 * Planning runs on the calling thread.  TQ_PLAN_THREADS=N (N > 1) lets a process-wide pool of N - 1
 * helper threads take slabs of a large batch; they touch only the call's own planner scratch and
 * the call returns after the last slab (off by default: no bench workload planned faster with it,
 * and a descheduled helper stalls the batch).
 * Streams: consecutive batches on one segment share its scratch buffers.  A batch enqueued on
 * another stream than the previous one first waits (stream-side, no host block) for that batch;
 * the host paths (tq_search_batch, tq_count_batch, tq_decode_*, tq_segment_set_alive_bitset,
 * tq_last_batch_*) wait for whatever the segment still has in flight on any stream.
 */
#ifndef TANTIVY_AMD_H
#define TANTIVY_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TQ_TERMINATED 0x7FFFFFFFu /* src/docset.rs:12 */
#define TQ_MAX_TERMS 16u          /* terms per device query */
#define TQ_MAX_K 1024u            /* largest per-segment k (offset+limit) the device heap holds */

enum tq_status {
  TQ_OK = 0,
  TQ_ERR_INVALID = 1,     /* bad argument */
  TQ_ERR_HIP = 2,         /* HIP runtime failure (maps to TantivyError::SystemError) */
  TQ_ERR_FORMAT = 3,      /* malformed index bytes (maps to TantivyError::DataCorruption) */
  TQ_ERR_UNSUPPORTED = 4, /* query shape the device path does not take (caller falls back) */
  TQ_ERR_NO_DEVICE = 5
};

/* IndexRecordOption of the *indexed* field (src/schema/index_record_option.rs); it fixes the
 * skip-entry size (5/8/12 B, src/postings/skip.rs:205-253). */
enum tq_record_option { TQ_BASIC = 0, TQ_WITH_FREQS = 1, TQ_WITH_FREQS_AND_POSITIONS = 2 };

/* Which executor the reference would pick (src/query/boolean_query/boolean_weight.rs:236-431):
 * AND    = all-Must term clauses   -> block_wand_intersection
 * OR     = all-Should term clauses -> block_wand / BufferedUnionScorer
 * PHRASE = PhraseQuery             -> PhraseScorer (tq_query.slop 0: the exact phrase; > 0: see "Sloppy phrases") */
enum tq_mode { TQ_MODE_AND = 0, TQ_MODE_OR = 1, TQ_MODE_PHRASE = 2, TQ_MODE_BOOL = 3 };
/* TQ_MODE_BOOL = BooleanQuery whose clauses are terms or BooleanQuerys of terms (unions of terms; since round 5
 * also nested intersections / exclusions / minimums: tq_query.nested_occurs), with mixed occurs
 * (`+a b -c`, `+a +(b OR c)`, `+(a OR b) +(c OR d)`) and minimum_number_should_match: the
 * Intersection / RequiredOptionalScorer / Exclude / Disjunction part of
 * BooleanWeight::complex_scorer (boolean_weight.rs:236-431, intersection.rs:20-56,
 * reqopt_scorer.rs:85-98, exclude.rs, disjunction.rs): docs = AND of the Must clauses (or OR of
 * the Should clauses when there is no Must), with at least min_should_match Should clauses
 * matching, minus the MustNot clauses; score = Must clauses summed cheapest first
 * (left + right + sum(others)) + the matching Should terms.  Values of tq_query.occurs follow
 * src/query/occur.rs. */
enum tq_occur { TQ_SHOULD = 0, TQ_MUST = 1, TQ_MUST_NOT = 2 };
/* tq_query.nested_occurs[i] | TQ_NESTED_PHRASE: the terms of the clause that share atom_of[i] are a PhraseQuery */
#define TQ_NESTED_PHRASE 0x10
/* tq_query.nested_occurs[i] | TQ_NESTED_ANY: the terms of the clause that share atom_of[i] are a UNION — a BooleanQuery
 * of Should terms one level further down, `(+(b c) +d) e`, `+a +(+(b c) +d)`: present where ANY of its terms is, scoring
 * the sum of the present ones (BufferedUnionScorer's SumCombiner) */
#define TQ_NESTED_ANY 0x20

typedef struct tq_ctx tq_ctx;
typedef struct tq_segment tq_segment;
typedef uint32_t tq_term_handle;
#define TQ_TERM_ABSENT 0xFFFFFFFFu /* term not in this segment (TermInfo lookup returned None) */
/* tq_query.terms[i] == TQ_TERM_ALL: clause i is an AllQuery (src/query/all_query.rs:23-112) — every doc below max_doc
 * matches (the alive filter applies as everywhere) and scores weights[i], its boost: 1.0 is a bare AllScorer, anything
 * else BoostScorer(AllScorer) (all_query.rs:24-31).  Allowed in TQ_MODE_AND (occur Must), TQ_MODE_OR (occur Should) and
 * flat TQ_MODE_BOOL, always as a clause of its own; TQ_MODE_PHRASE: TQ_ERR_INVALID; sharing a clause_of value with
 * another entry or inside a nested query: TQ_ERR_UNSUPPORTED.  What the query then is — BooleanWeight::complex_scorer
 * read literally (boolean_weight.rs:114-171, 236-431, 440-456) — is decided by tq_all_query_form below (DESIGN.md
 * "AllQuery"): EMPTY, PLAIN (the All clauses vanish without a trace, scores included: `+* +a` scores bm25(a)) or
 * ALL-BASED (every doc, or the docs with at least min_should Should clauses, minus the MustNot lists; score = the sum
 * of the present Should clauses + 1.0 however many All clauses there were).  A boosted All (weights[i] != 1.0) is
 * taken by the scoring entry points only as the sole non-MustNot clause that holds anything (`*^b`, `+*^b -a`); doc
 * sets and counts do not depend on the boost. */
#define TQ_TERM_ALL 0xFFFFFFFEu

/* One query against one segment.  Replaces the per-segment scorer tree the reference builds in
 * BooleanWeight::complex_scorer / TermWeight::specialized_scorer / PhraseWeight::phrase_scorer.
 * The BM25 statistics are computed by the caller from *global* (cross-segment) counts exactly as
 * Bm25Weight::for_terms does (src/query/bm25.rs:95-129): */
typedef struct tq_query {
  uint32_t n_terms;              /* 1..TQ_MAX_TERMS */
  const tq_term_handle *terms;   /* from tq_term_prepare, or TQ_TERM_ABSENT */
  const float *weights;          /* AND/OR: n_terms x (idf*(1+K1)*boost); PHRASE: weights[0] */
  const float *tf_cache;         /* Bm25Weight.cache: 256 f32, K1*(1-B+B*fieldnorm/avg) */
  uint8_t mode;                  /* enum tq_mode */
  const uint32_t *phrase_offsets; /* PHRASE: term offsets inside the phrase; BOOL with phrase atoms: per term; else NULL */
  uint32_t k;                    /* TopDocs offset+limit, 1..TQ_MAX_K */
  const uint8_t *occurs;         /* TQ_MODE_BOOL: n_terms x enum tq_occur; else NULL */
  const uint8_t *clause_of;      /* TQ_MODE_BOOL: clause index per term (terms sharing a value form
                                    one nested all-Should BooleanQuery, `+a +(b OR c)`); NULL =
                                    every term is its own clause */
  uint32_t min_should_match;     /* TQ_MODE_BOOL: BooleanQuery::minimum_number_should_match */
  uint32_t slop;                 /* TQ_MODE_PHRASE: PhraseQuery::set_slop, 0..TQ_MAX_SLOP (see "Sloppy phrases" below); any
                                    other mode: must be 0 (TQ_ERR_INVALID naming the query).  The field sits in what was
                                    padding in front of the next pointer: sizeof(tq_query) and every other offset are
                                    unchanged, and CALLERS MUST ZERO THE STRUCT (a zeroed query has slop 0) */
  /* TQ_MODE_BOOL, one level of nesting beyond unions of terms (round 5): a clause_of group is a nested
   * BooleanQuery of terms, every term with its own occur INSIDE it — `+a +(+b +c)`, `(+b +c) d`, `+a -(+b +c)`,
   * `+a +(+b c -d)` — and its own minimum_number_should_match.  Both NULL (or every nested occur TQ_SHOULD and every
   * nested minimum <= 1) = unions of terms as before.  Evaluated over the lists' bitmaps (TQ_KERNEL_TREE). */
  const uint8_t *nested_occurs;      /* n_terms x enum tq_occur: the term's occur inside its clause_of group; or NULL */
  const uint8_t *clause_min_should;  /* TQ_MAX_TERMS entries indexed by clause_of value: the nested query's
                                        minimum_number_should_match; or NULL */
  const uint8_t *atom_of;            /* n_terms values, or NULL: terms of one clause_of group that share an atom_of
                                        value form a CONJUNCTION — a BooleanQuery of Must terms one level further down,
                                        `+a +((+b +c) d)`: present where all its terms are, scoring their sum; its occur
                                        inside the group is nested_occurs of its terms (equal for all of them).  NULL =
                                        every term is its own member of its group.
                                        A PHRASE inside the boolean query (`+"a b" +c`, `"a b" c`, `+c -"a b"`,
                                        `+a +("b c" d)`; PhraseQuery as a clause of BooleanQuery: PhraseScorer under
                                        Intersection / union / Exclude, phrase_scorer.rs:347-587): the terms of the
                                        phrase share an atom_of value, carry nested_occurs | TQ_NESTED_PHRASE, their
                                        phrase_offsets[i] (0 on the other terms) and — each of them — the PHRASE's
                                        weight ((1 + K1) * boost * sum of idfs) in weights[i].  2..8 terms per phrase; a
                                        phrase that is a clause of its own is a clause_of group of one atom.
                                        A UNION one level further down (nested_occurs | TQ_NESTED_ANY, round 6): see above. */
} tq_query;
#ifdef __cplusplus
static_assert(sizeof(void *) != 8 || (sizeof(tq_query) == 104 && offsetof(tq_query, nested_occurs) == 80 &&
                                      offsetof(tq_query, slop) == offsetof(tq_query, min_should_match) + 4),
              "tq_query.slop fills the padding behind min_should_match: the layout of the struct is unchanged");
#endif

/* ---- Sloppy phrases (TQ_MODE_PHRASE with slop > 0) ----
 * slop 0 is the exact phrase: the kernels and kernel_mask it always had.  slop > 0 runs as TQ_KERNEL_PHRASE_SLOP, a
 * launch group of its own over the lists' bitmaps (every list through a bitmap + rank directory, its own or the probe
 * pool's, as for TQ_KERNEL_TREE: "use_dense" off or tables outside one 32 GB span is TQ_ERR_UNSUPPORTED), nothing
 * pruned: "exhaustive" 0 and 1 give the same rows and tq_last_batch_match_counts is the number of matching docs.
 * Validation as for any phrase (2..8 terms, phrase_offsets, a field with positions, a finite weight; an absent term is
 * an empty result).  The device restates the reference's algorithm, which is NOT "an exact phrase with a window":
 *  - the lists are walked in COST order (doc freq ascending, ties in phrase order), and with slop that order changes
 *    verdicts and counts;
 *  - SCORED and UNSCORED verdicts differ for 3 and more terms: tq_search_batch* / tq_submit / tq_search_one count
 *    matches carrying the slop already spent (doc `a x b x c`, phrase "a b c"~1: no match); tq_count_batch and
 *    tq_docset_batch* (under "docset_trees" = 1; refused without it as phrases are) test the last term without it
 *    (the same doc matches) — exactly as the reference's scoring and non-scoring PhraseScorer do;
 *  - for 3 and more terms the reference carries a list of (position, slop spent) that has no bound.  The device keeps
 *    TQ_SLOP_CARRY_CAP entries per candidate doc.  A doc whose initial or carried list would exceed that bumps the
 *    query's OVERFLOW word and its verdict is unspecified: the host-output entry points (tq_search_batch[_opts],
 *    tq_count_batch, host tq_docset_batch) then return TQ_ERR_UNSUPPORTED naming the first such query ("carried position
 *    list over TQ_SLOP_CARRY_CAP") — the caller falls back for it; the other queries' rows are written and valid.
 *    tq_submit / tq_wait / tq_search_one fail the overflowing query's ticket alone.  Callers of the _device variants MUST
 *    read tq_last_batch_slop_overflows for batches that hold a sloppy phrase of 3 or more terms.  A 2-term phrase never
 *    overflows.
 * Refused (TQ_ERR_UNSUPPORTED naming the query, nothing launched, the segment usable): slop > TQ_MAX_SLOP;
 * tq_docset_scored_batch* with a sloppy phrase (also under "docset_score_trees"); a sloppy phrase over terms of a field
 * other than 0.  A phrase ATOM inside a TQ_MODE_BOOL query cannot carry a slop: there is one slop per query and only
 * TQ_MODE_PHRASE reads it.
 * algorithmic_bytes of such a query is a MODEL, not a measurement: (lists + 1) x bitmap words x 4, (lists + 2) where a
 * result bitmap is written (once, by the sloppy-phrase kernel itself) and read back (doc sets, counts); positions are not
 * counted. */
#define TQ_MAX_SLOP 255u /* the reference keeps the slop spent in a u8: above 255 its cast wraps, and nobody should depend on that */
/* Entries of a carried list the device keeps per candidate doc (two lists per lane in LDS: 64 lanes x 2 x 32 x (4 + 1)
 * bytes = 20 KB per workgroup, 8 workgroups per CU of 160 KB; random docs of tf <= 8, 3..8 terms, slop <= 8 reached 27) */
#define TQ_SLOP_CARRY_CAP 32u

/* The normal form of a query with TQ_TERM_ALL clauses (pure: needs no segment; handles other than TQ_TERM_ALL /
 * TQ_TERM_ABSENT count as present lists).  kind: TQ_ALL_EMPTY = no doc matches; TQ_ALL_PLAIN = the query is its
 * entries in keep_mask with minimum_number_should_match = min_should, evaluated as a query without All clauses is;
 * TQ_ALL_BASED = the doc set is every doc (min_should == 0) or the docs that hold at least min_should of the Should
 * clauses in keep_mask, minus the MustNot lists in keep_mask, and the score is the sum of the present Should clauses
 * + base.  keep_mask: bit i = entry i holds a list that survives (0 for TQ_ALL_EMPTY).  Returns TQ_ERR_INVALID for
 * null arguments, a malformed query, an All clause in a phrase or a non-finite boost; TQ_ERR_UNSUPPORTED for an All
 * clause inside a nested query or a clause_of union, and for a boosted All beside another scoring clause or a second
 * All — `out` then still holds the doc-set form (which the boost does not change) with base = NaN.
 * weights == NULL: every boost is 1.0. */
enum tq_all_kind { TQ_ALL_EMPTY = 0, TQ_ALL_PLAIN = 1, TQ_ALL_BASED = 2 };
typedef struct tq_all_form {
  uint32_t kind;       /* enum tq_all_kind */
  float base;          /* TQ_ALL_BASED: the score every doc of the set starts from */
  uint32_t min_should; /* the minimum left after the Should-All clauses were counted off */
  uint32_t keep_mask;
} tq_all_form;
int tq_all_query_form(const tq_query *q, tq_all_form *out);

/* ---- lifecycle ---- */
/* replaces: nothing in the reference (device bring-up).  device_ids==NULL => {0}. */
int tq_init(const int *device_ids, int n_devices, tq_ctx **out);
void tq_shutdown(tq_ctx *ctx);
const char *tq_last_error(void);

/* ---- segment residency ----
 * replaces: SegmentReader::inverted_index(field) + InvertedIndexReader::new
 * (src/index/segment_reader.rs:221-283, src/index/inverted_index_reader.rs:66-81) and
 * FieldNormReader::open (src/fieldnorm/reader.rs:99-105): the field's raw sub-files are copied
 * to HBM unchanged.  idx = the field's `.idx` sub-file including its 8-byte total_num_tokens
 * header; pos = the field's `.pos` sub-file (NULL if no positions); fieldnorm = max_doc bytes
 * (NULL => FieldNormReader::constant(max_doc, 1), src/query/term_query/term_weight.rs:209-219).
 * The natural caller is a Warmer (src/reader/warming.rs:14-20). */
int tq_segment_upload(tq_ctx *ctx, int device, uint32_t max_doc, const uint8_t *idx,
                      size_t idx_len, const uint8_t *pos, size_t pos_len,
                      const uint8_t *fieldnorm, size_t fn_len, uint8_t record_option,
                      tq_segment **out);
/* The same for sub-files that are ALREADY in device memory on `device` (written by
 * tq_encode_postings_device / tq_encode_positions_device, or copied there by the caller): the
 * bytes are copied device to device and the library keeps no host copy — tq_term_prepare then
 * walks skip lists and positions headers in HBM (tq_prepare.hip) and builds the dense-list
 * tables with device scans; only a few dozen bytes of facts per term cross back to the host.
 * d_idx includes the 8-byte total_num_tokens header like idx above. */
int tq_segment_upload_device(tq_ctx *ctx, int device, uint32_t max_doc, const uint8_t *d_idx,
                             size_t idx_len, const uint8_t *d_pos, size_t pos_len,
                             const uint8_t *d_fieldnorm, size_t fn_len, uint8_t record_option,
                             tq_segment **out);
void tq_segment_free(tq_segment *seg);

/* ---- multi-field segments ----
 * replaces: one SegmentReader::inverted_index(field) + fieldnorms_readers().get_field(field) per indexed Field of a
 * query (src/index/segment_reader.rs:221-283, src/query/term_query/term_weight.rs:196-219): F >= 1 fields over ONE
 * doc-id space, queries whose terms come from any of them — what QueryParser makes of `hello world` over the default
 * fields [title, body]: (title:hello body:hello) (title:world body:world).  Every term scores with its OWN field's
 * fieldnorm and its own field's Bm25Weight cache.
 * fields[f] = the sub-files of field f, with the meaning of tq_segment_upload's arguments (fieldnorm NULL: that
 * field reads FieldNormReader::constant(max_doc, 1)); all fields share one record_option (the skip-entry size depends
 * on it; per-field options are not taken).  1 <= n_fields <= TQ_MAX_FIELDS, else TQ_ERR_INVALID; n_fields == 1 is
 * tq_segment_upload.  There is no device-resident variant.
 * Layout: the fields' .idx sub-files are laid end to end (each with its 8-byte header and its padding) in one device
 * buffer, the .pos sub-files in another; a term's offsets are shifted by its field's base when it is prepared, and
 * every decode path reads the shifted offsets unchanged.  Field 0's fieldnorms lie where a single-field segment's do;
 * fields 1.. add max_doc bytes each (tq_fields_stats.extra_fieldnorm_bytes).
 * FIELD 0 IS THE PRIMARY FIELD: the doc matrix's fieldnorm byte, the lists' range maxima / list maxima / leader
 * norms, the segment's own Bm25Weight cache, and with them the shared and the pruned kernels, are field 0's.  A
 * query that names only field-0 terms runs exactly as on a single-field upload of field 0: same kernels, same rows.
 * Lists of a field != 0 get bitmaps, tf bytes, position directories, doc-matrix columns / signature bits and range
 * directories like any list (membership and tf only) and none of the norm-derived tables.
 * Queries on a segment with F > 1: tq_query.tf_cache points at F x 256 floats, row f = Bm25Weight.cache under field
 * f's average fieldnorm; weights stay per term (idf from that field's statistics, Bm25Weight::for_terms per
 * TermQuery).  F == 1: nothing changes.
 *   tq_count_batch, tq_docset_batch*   bitmap words and positions only: any field mix, "docset_trees" shapes included
 *   tq_search_batch*, tq_submit / tq_search_one
 *                             a query naming at least one term of a field != 0 runs as TQ_KERNEL_TREE whatever its mode
 *                             (tree_fields_kernel, tq_tree_fields.hip: per-LIST norms), occurs on call scratch as for
 *                             term sets; nothing is pruned, "exhaustive" 0 and 1 give the same rows and
 *                             tq_last_batch_match_counts is the doc-set size; refusals as for any tree ("use_dense" off,
 *                             tables outside one 32 GB span, a negative weight: TQ_ERR_UNSUPPORTED).  TQ_MODE_AND / OR /
 *                             BOOL with clause_of unions, nested shapes, phrase atoms (scored with the norm of their
 *                             terms' field), term sets beside them; a TQ_MODE_PHRASE query of one field f != 0 runs as
 *                             a one-atom tree.  A phrase or phrase atom whose terms are of DIFFERENT fields:
 *                             TQ_ERR_INVALID naming the query (the reference's PhraseQuery panics on it).  A term set
 *                             with members of different fields is fine: a bitmap and a constant.  TQ_TERM_ALL beside
 *                             field terms is taken where it is taken today with ONE exception: a Should term of a
 *                             field != 0 in a query that its All clauses make ALL-BASED (such a query keeps Should and
 *                             MustNot lists only: its Should terms are what scores) is TQ_ERR_UNSUPPORTED (all_kernel scores under the primary field's norms; MustNot terms of
 *                             any field are taken: bits only; EMPTY / PLAIN forms run as the stripped query does).
 *   tq_docset_scored_batch*   flat shapes take any field mix (docset_score_fields_kernel, tq_docset_score_fields.hip: per-list
 *                             norms, the same sums).  Under "docset_score_trees", a phrase or a nested query that names a
 *                             term of a field != 0: TQ_ERR_UNSUPPORTED naming the query in this version, nothing launched
 *                             (the parser's shape is flat and is taken).
 * tq_segment_reserve_columns names field-0 lists. */
#define TQ_MAX_FIELDS 8u
typedef struct tq_field_files {
  const uint8_t *idx;
  size_t idx_len;
  const uint8_t *pos; /* NULL: no positions */
  size_t pos_len;
  const uint8_t *fieldnorm; /* NULL: FieldNormReader::constant(max_doc, 1) */
  size_t fn_len;
} tq_field_files;
int tq_segment_upload_fields(tq_ctx *ctx, int device, uint32_t max_doc, uint32_t n_fields,
                             const tq_field_files *fields, uint8_t record_option, tq_segment **out);
typedef struct tq_fields_stats {
  uint32_t n_fields;
  uint32_t n_field_terms;            /* prepared terms of fields != 0 (0: no entry point looks at a query's fields) */
  uint64_t extra_fieldnorm_bytes;    /* fieldnorm bytes of fields 1.. (field 0's: tq_segment_stats.fieldnorm_bytes) */
} tq_fields_stats;
int tq_segment_get_fields_stats(tq_segment *seg, tq_fields_stats *out);

/* replaces: InvertedIndexReader::read_postings_from_terminfo + BlockSegmentPostings::open +
 * SkipReader::new + PositionReader::open (inverted_index_reader.rs:204-247,
 * block_segment_postings.rs:97-140, skip.rs:131-151, positions/reader.rs:43-56).
 * Arguments are the fields of TermInfo (src/postings/term_info.rs:10-17): ranges are relative to
 * the sub-file body (after the 8-byte header for .idx).  Walks the sequential skip list once and
 * keeps it on the device as a random-access table; idempotent per (postings_off). */
int tq_term_prepare(tq_segment *seg, uint64_t postings_off, uint32_t postings_len,
                    uint64_t positions_off, uint32_t positions_len, uint32_t doc_freq,
                    tq_term_handle *out);
/* The same for many terms at once (the new terms of a query batch): one staged upload, one wait, one launch for the
 * doc signatures of the lists without a column — tq_term_prepare costs a blocking copy and two launches per term.
 * infos[i] = the fields of the term's TermInfo (postings/term_info.rs:10-17); out[i] = its handle (terms already
 * prepared: the handle they have).  Replaces n calls of InvertedIndexReader::read_block_postings_from_terminfo
 * (src/index/inverted_index_reader.rs:204-247) + BlockSegmentPostings::open (block_segment_postings.rs:97-140). */
typedef struct tq_term_info {
  uint64_t postings_off;
  uint64_t positions_off;
  uint32_t postings_len, positions_len;
  uint32_t doc_freq;
  uint32_t pad_;
} tq_term_info;
int tq_term_prepare_batch(tq_segment *seg, const tq_term_info *infos, uint32_t n, tq_term_handle *out);
/* The same for a term of field `field` of a multi-field segment (tq_segment_upload_fields): the offsets are relative
 * to THAT field's sub-file bodies, the library adds the field's base.  tq_term_prepare / tq_term_prepare_batch mean
 * field 0.  Idempotent per (field, postings_off): the same postings_off in two fields gives two handles.
 * field >= the segment's field count: TQ_ERR_INVALID.  fields = n bytes, one per info. */
int tq_term_prepare_field(tq_segment *seg, uint32_t field, uint64_t postings_off, uint32_t postings_len,
                          uint64_t positions_off, uint32_t positions_len, uint32_t doc_freq,
                          tq_term_handle *out);
int tq_term_prepare_batch_fields(tq_segment *seg, const tq_term_info *infos, const uint8_t *fields, uint32_t n,
                                 tq_term_handle *out);
/* *field = the field the handle's list belongs to (a term set: 0). */
int tq_term_field(tq_segment *seg, tq_term_handle term, uint32_t *field);
/* Optional, before the first tq_term_prepare: names the posting lists (by postings_off) that get
 * the 40 columns of the segment's doc matrix — the caller knows every term's doc_freq from the
 * term dictionary and passes the densest lists.  Without it the columns go to the first 40 dense
 * lists that happen to be prepared, i.e. the layout (and 5..15 % of the union kernels' time)
 * depends on the order of the first queries.  Lists beyond the 40 named are ignored. */
int tq_segment_reserve_columns(tq_segment *seg, const uint64_t *postings_offs, uint32_t n);

/* ---- term sets ----
 * replaces: the bitset loop of AutomatonWeight::scorer (src/query/automaton_weight.rs:87-111) for one segment — what
 * FuzzyTermQuery, RegexQuery, TermSetQuery and every other AutomatonWeight query do: the docs of N posting lists OR-ed
 * into a BitSet(max_doc) under ConstScorer(BitSetDocSet, boost) (src/query/const_score_query.rs:95-148,
 * src/query/bitset/mod.rs:91-93).  members = n handles from tq_term_prepare(_batch) — the caller gets their TermInfos
 * from its own term stream, exactly where the reference does; TQ_TERM_ABSENT members and duplicates are skipped; n == 0
 * or no present member gives a valid handle with an empty bitmap (the reference keeps a ConstScorer over an empty
 * bitset, not an EmptyScorer); a member that is TQ_TERM_ALL, a set, out of range or released: TQ_ERR_INVALID.  n up to
 * 2^20.  Built on the segment's stream (tq_termset.hip): members with a bitmap are OR-ed word-wise in one launch, the
 * others scattered block by block, a device scan writes the rank directory; the call returns once the set's doc count
 * is known (one small blocking copy).  The members stay what they were.
 * The result is a {32 doc bits, docs before the word} table of ceil(max_doc / 32) words — the layout of the dense
 * lists' bitmaps, read unchanged by every bitmap kernel — counted in tq_segment_stats.bitmap_bytes but NOT against
 * "dense_budget_x" (which ordinary lists get bitmaps does not depend on sets).  Deleted docs are in it, as in the
 * reference's bitset; the alive filter applies where it always does.
 * The handle is a slot of the segment's term table and an entry of tq_query.terms like any other.  Wherever the set is
 * present it scores weights[i] AS GIVEN — the caller passes boost, or boost * score for ConstScoreQuery: no BM25, no
 * fieldnorm, no tf; its cost, wherever clauses are sorted by cost, is its doc count (BitSet::len: the reference's
 * size_hint).  Allowed in TQ_MODE_AND, TQ_MODE_OR and flat TQ_MODE_BOOL, also as one of several entries sharing a
 * clause_of value (`+a +(b OR set)`), several sets per query.
 *   tq_count_batch            never a scan: count_bitmap_kernel whatever "count_bitmap_ratio" says, the doc-set count
 *                             pass for "at least m of n"
 *   tq_docset_batch*          the set's table is one more bitmap of the expression
 *   tq_docset_scored_batch*   presence from the bitmap word, score = weights[i], summed in the usual order
 *   tq_search_batch*, tq_submit / tq_search_one: the reference takes the generic unpruned scorer path as soon as one
 *                             scorer of a query is not a TermScorer (boolean_weight.rs:44-86); here the query runs as
 *                             TQ_KERNEL_TREE whatever its mode, its other lists reached through bitmaps (their own or
 *                             the probe pool's) — "use_dense" off, tables outside one 32 GB span or a negative weight:
 *                             TQ_ERR_UNSUPPORTED as for any tree.  Nothing is pruned: "exhaustive" 0 and 1 give the same
 *                             rows and tq_last_batch_match_counts is the doc-set size.
 *   beside TQ_TERM_ALL        counts and (scored) doc sets take sets in any role; top-k takes them as MustNot lists
 *                             (`+* -set`); a Should set beside an All clause in tq_search_batch*: TQ_ERR_UNSUPPORTED
 * Refused, with the query index in tq_last_error(), nothing launched and the segment usable: a set in TQ_MODE_PHRASE or
 * carrying TQ_NESTED_PHRASE (TQ_ERR_INVALID); a set in a query with nested_occurs / atom_of structure
 * (TQ_ERR_UNSUPPORTED); tq_decode_postings / tq_decode_position_deltas of a set (TQ_ERR_INVALID).
 * In algorithmic_bytes / unique_bytes a set enters, wherever a list enters with its postings_len, with
 * ceil(max_doc / 32) * 4.
 * With the option "timing" set tq_term_set_prepare leaves the build in the segment's tq_batch_stats for
 * tq_last_batch_stats, in place of the last batch's figures: kernel_ms = total_ms = the HIP-event time from the zeroing of
 * the table to the end of the rank pass, algorithmic_bytes = the build's HBM model (the scattered members' posting bytes
 * + 4 B per 32 docs per member with a bitmap + 8 B per 32 docs written and read once by the scan), chunks = the members
 * that were OR-ed word-wise (the others were scattered), batches_averaged = 1, everything else 0. */
int tq_term_set_prepare(tq_segment *seg, const tq_term_handle *members, uint32_t n, tq_term_handle *out);
/* *n_docs = docs in the set (deleted ones included), *bytes = its resident bytes, ceil(max_doc / 32) * 8. */
int tq_term_set_info(tq_segment *seg, tq_term_handle set, uint32_t *n_docs, uint64_t *bytes);
/* Waits for whatever the segment has in flight on any stream, returns the table and tombstones the slot: a query, a
 * member list or an info / release call that names it afterwards gets TQ_ERR_INVALID; a later tq_term_set_prepare may
 * reuse the slot.  tq_segment_free frees the sets still outstanding. */
int tq_term_set_release(tq_segment *seg, tq_term_handle set);

/* ---- fast-field ranges ----
 * replaces: FastFieldRangeWeight::scorer for a u64-mapped fast field (src/query/range_query/range_query_fastfield.rs:
 * 54-239 -> search_on_u64_ff :414-450 -> RangeDocSet over a Column<u64> under ConstScorer(docset, boost),
 * fast_field_range_doc_set.rs) for one segment: `+body:error +timestamp:[a TO b]`, `price:[10 TO 20]`,
 * `* -age:{* TO 18}`.
 * A COLUMN is one serialized u64_based column-values blob, byte for byte as serialize_u64_based_column_values writes it
 * (columnar/src/column_values/u64_based/mod.rs:79-110): a codec byte (0 Bitpacked, 1 Linear, 2 BlockwiseLinear),
 * ColumnStats as four VInts — min, gcd, amplitude / gcd, num_rows (stats.rs:30-54; common's VInt, stop bit on the LAST
 * byte) — and the codec's payload (bitpacked.rs, linear.rs, blockwise_linear.rs, line.rs, bitpacker/src/bitpacker.rs).
 * The payload stays in HBM as the file holds it, in a 256-byte-aligned buffer of its own with 16 zero bytes behind it;
 * BlockwiseLinear adds one 32-byte record per block of 512 rows (slope, intercept, data offset, bit width).  Up to
 * TQ_MAX_COLUMNS columns per segment; their bytes are tq_column_info_t.resident_bytes, not part of tq_segment_stats.
 *   TQ_CARD_FULL         present_words must be NULL and num_rows == max_doc (else TQ_ERR_FORMAT): a doc's row is the doc
 *   TQ_CARD_OPTIONAL     present_words = ceil(max_doc / 32) words, bit d of the array set when doc d has a value (the
 *                        caller reads them off the reference's OptionalIndex); bits at or above max_doc are ignored; their
 *                        popcount must be num_rows (else TQ_ERR_FORMAT); a doc's row is the number of set bits below it
 *   TQ_CARD_MULTIVALUED  TQ_ERR_UNSUPPORTED in this version
 * Malformed bytes — truncated anywhere, an unknown codec byte, gcd 0, min + amplitude past u64, a bit width of 57..63 or
 * above 64, a payload shorter than ceil(num_rows * num_bits / 8), a BlockwiseLinear footer that does not fit — are
 * TQ_ERR_FORMAT with a message, never a crash.  tq_column_parse is that check alone, on the host, without a device: it
 * fills codec, min, max, gcd, num_rows, num_bits (resident_bytes = what an upload would hold, cardinality 0).
 *
 * tq_range_prepare turns (column, value range) into a TERM-SET handle (above): a {32 doc bits, docs before the word} table
 * built by tq_range.hip — a lane per doc reads its row's packed value and compares it with the range divided by the gcd
 * (transform_range_before_linear_transformation, bitpacked.rs:37-49), a wavefront's ballot is two words of the table,
 * the term sets' rank stage follows — that tq_term_set_info, tq_term_set_release, tq_term_table_read(TQ_TABLE_DENSE) and
 * every query entry point treat exactly as a term set, refusals included (phrases, nested structure, a Should set beside
 * an All clause in top-k).  It scores *out_weight wherever it is present: pass that as the entry's weight.  Releasing the
 * column does not touch handles already built from it.
 * The bounds are in the column's u64 space: the caller applies MonotonicallyMappableToU64 first (u64: the value; i64:
 * (uint64_t)v ^ (1 << 63); f64: bits ^ (bits >> 63 ? ~0 : 1 << 63); bool: 0 / 1; date: its i64 of nanoseconds) and the
 * JSON numeric coercions of :254-412.  Then search_on_u64_ff + bound_to_value_range + RangeDocSet::new, literally:
 *   both bounds unbounded     *out = TQ_TERM_ALL, *out_weight = 1.0f (the reference returns AllScorer before it looks at
 *                             the column, and drops the boost, :57-59); the column is not looked at
 *   start / end               start = lower, lower + 1 for Excluded (overflow: empty), the column's min when unbounded, then
 *                             raised to min; end = upper, upper - 1 for Excluded (underflow: empty), max when unbounded,
 *                             NOT clamped
 *   empty                     start > end, start > max, end < min or num_rows == 0: a valid handle over a zeroed table (no
 *                             kernel runs), 0 docs, *out_weight = boost
 *   full coverage             min >= start && max <= end on a TQ_CARD_FULL column: boost == 1.0f gives *out = TQ_TERM_ALL,
 *                             *out_weight = 1.0f (an AllScorer: `+range +a` scores bm25(a) alone); any other boost a set
 *                             of all max_doc docs scoring boost.  An Optional column never takes the shortcut (:443-445)
 *   otherwise                 the fill; *out_weight = boost
 * A bound kind above TQ_BOUND_EXCLUDED, a column that is out of range or released (unless both bounds are unbounded):
 * TQ_ERR_INVALID.  With the option "timing" set the build's figures replace the last batch's, as after
 * tq_term_set_prepare: kernel_ms = total_ms = from the zeroing to the end of the rank stage, algorithmic_bytes = the
 * payload's bytes + 16 B per 32 docs (the table written, and read once by the scan) + 8 B per 32 docs of presence table
 * of an Optional column; an empty range: 0 bytes. */
#define TQ_MAX_COLUMNS 16u
enum tq_cardinality { TQ_CARD_FULL = 0, TQ_CARD_OPTIONAL = 1, TQ_CARD_MULTIVALUED = 2 };
enum tq_column_codec { TQ_CODEC_BITPACKED = 0, TQ_CODEC_LINEAR = 1, TQ_CODEC_BLOCKWISE_LINEAR = 2 };
enum tq_bound_kind { TQ_BOUND_UNBOUNDED = 0, TQ_BOUND_INCLUDED = 1, TQ_BOUND_EXCLUDED = 2 };
typedef struct tq_column_info_t {
  uint64_t min_value, max_value, gcd;
  uint64_t resident_bytes; /* payload + padding, block records, presence table */
  uint32_t num_rows;
  uint32_t num_bits;       /* Bitpacked: bits per value (0..56 or 64); the linear codecs: 0 */
  uint32_t codec;          /* tq_column_codec */
  uint32_t cardinality;    /* tq_cardinality */
} tq_column_info_t;
int tq_column_parse(const uint8_t *values, size_t values_len, tq_column_info_t *out);
int tq_column_upload(tq_segment *seg, const uint8_t *values, size_t values_len, uint8_t cardinality,
                     const uint32_t *present_words, uint32_t *out_column);
int tq_column_info(tq_segment *seg, uint32_t column, tq_column_info_t *out);
/* Waits for the segment to be idle, like tq_term_set_release, and frees the column's buffers; the slot is taken by a
 * later upload.  tq_segment_free frees the columns still held. */
int tq_column_release(tq_segment *seg, uint32_t column);
/* Codec access (tests, tooling): out_host[i] = the value of ROW first_row + i, i < n — min + gcd * n for Bitpacked and
 * BlockwiseLinear, line.eval(row) + diff for Linear — read by the kernels' own three readers.  first_row + n > num_rows:
 * TQ_ERR_INVALID. */
int tq_column_decode(tq_segment *seg, uint32_t column, uint32_t first_row, uint32_t n, uint64_t *out_host);
int tq_range_prepare(tq_segment *seg, uint32_t column, uint8_t lower_kind, uint64_t lower, uint8_t upper_kind, uint64_t upper,
                     float boost, tq_term_handle *out, float *out_weight);

/* ---- search ----
 * replaces, for each query: TopBySortKeyCollector::collect_segment ->
 * SortBySimilarityScore::collect_segment_top_k -> Weight::for_each_pruning -> {block_wand,
 * block_wand_intersection, for_each_pruning_scorer(PhraseScorer)} -> TopNHeap
 * (src/collector/sort_key_top_collector.rs:62-73, sort_key/sort_by_score.rs:35-161,
 *  src/query/boolean_query/{block_wand_union,block_wand_intersection}.rs,
 *  src/query/phrase_query/phrase_scorer.rs).
 * Output per query q (row stride = out_stride >= max k): the segment's top-k sorted by
 * (score desc, doc asc) — i.e. TopNHeap::into_vec after the sort merge_top_k applies — padded
 * with (0.0, TQ_TERMINATED); out_counts[q] = number of real hits.  Host buffers. */
int tq_search_batch(tq_segment *seg, const tq_query *queries, uint32_t n_queries,
                    uint32_t out_stride, float *out_scores, uint32_t *out_docs,
                    uint32_t *out_counts);

/* Same, but the outputs are DEVICE pointers on the segment's device and the call only enqueues
 * work on `hip_stream` (a hipStream_t; NULL = the segment's own stream) without a final host
 * synchronisation — for callers that feed an RCCL all-gather (tq_merge_topk_device) next. */
int tq_search_batch_device(tq_segment *seg, const tq_query *queries, uint32_t n_queries,
                           uint32_t out_stride, float *d_out_scores, uint32_t *d_out_docs,
                           uint32_t *d_out_counts, void *hip_stream);

/* Per-call execution options: everything a call needs that is not part of the queries.  Carried
 * per call (not as segment state) so that two Searchers / threads sharing the statistics of
 * different indexes never race on a segment's options.
 *   exhaustive       -1 = the segment's "exhaustive" option (tq_set_option), 0 = block-max pruning
 *                    as block_wand / block_wand_intersection do, 1 = score every match
 *   bound_slack_ppm  TQ_OPT_DEFAULT = the segment's option; else block-max bounds are widened by
 *                    (1 + ppm * 1e-6) for THIS call.  Callers whose Bm25Weights come from global
 *                    (cross-segment) statistics MUST pass ((1 + d)^2 - 1) * 1e6 with d = the
 *                    relative difference between the global and this segment's average
 *                    fieldnorm, or pruning is only as exact as the reference's own
 *                    (term_scorer.rs:58-70); the host mirror (Searcher) does. */
#define TQ_OPT_DEFAULT 0xFFFFFFFFu
typedef struct tq_search_opts {
  int32_t exhaustive;
  uint32_t bound_slack_ppm;
} tq_search_opts;
/* tq_search_batch / tq_search_batch_device with per-call options (opts == NULL: segment defaults). */
int tq_search_batch_opts(tq_segment *seg, const tq_query *queries, uint32_t n_queries,
                         uint32_t out_stride, float *out_scores, uint32_t *out_docs,
                         uint32_t *out_counts, const tq_search_opts *opts);
int tq_search_batch_device_opts(tq_segment *seg, const tq_query *queries, uint32_t n_queries,
                                uint32_t out_stride, float *d_out_scores, uint32_t *d_out_docs,
                                uint32_t *d_out_counts, const tq_search_opts *opts,
                                void *hip_stream);
/* tq_search_batch_device_opts for an index of ONE segment: the rows are merge_top_k's already (it orders one segment's
 * hits by score desc, doc asc), so the batch's merge kernels write its column of segment ordinals as well —
 * d_out_segment_ords[q][i] = segment_ord for i < d_out_counts[q], 0xFFFFFFFF in the padding — and the caller needs no
 * tq_merge_topk_device launch and no intermediate slab.  With out_stride = k of every query the four arrays are, bit for
 * bit, what tq_merge_topk_device(offset 0, limit k) makes of tq_search_batch_device_opts' (DESIGN.md §5 has the one
 * caveat: a row holding both +0.0 and -0.0 scores).  Outputs: device memory, or pinned host memory mapped into the device. */
int tq_search_batch_device_rows(tq_segment *seg, const tq_query *queries, uint32_t n_queries,
                                uint32_t out_stride, float *d_out_scores, uint32_t *d_out_segment_ords,
                                uint32_t *d_out_docs, uint32_t *d_out_counts, uint32_t segment_ord,
                                const tq_search_opts *opts, void *hip_stream);

/* ---- concurrent single-query entry (tantivy's own call pattern) ----
 * replaces: Collector::collect_segment(&dyn Weight, segment_ord, &SegmentReader) as
 * Searcher::search_with_executor calls it — from any number of threads at once, one query per call
 * (src/core/searcher.rs:180-238, src/collector/mod.rs:173-183; `Weight: Send + Sync`,
 * src/query/weight.rs:66).  One query per launch is the ~0.3 ms regime of the device; these entry
 * points coalesce the single queries of concurrent callers into the batched launch:
 *   tq_submit      puts one query on the segment's pending list and returns a ticket.  The query's
 *                  arrays (terms, weights, tf_cache, ...) and the output buffers (k scores / docs,
 *                  one count) are borrowed until tq_wait returns.
 *   tq_wait        blocks until the launch that carried the query has finished and frees the
 *                  ticket.  Whoever waits while no batch is running LEADS the next one: it takes
 *                  everything pending that runs under the same options, issues ONE tq_search_batch
 *                  for it and hands every caller its rows (callers keep arriving while the previous
 *                  batch runs — nobody waits for a batch to fill).  Work only happens inside
 *                  tq_wait: a ticket that is never waited for is never run (and leaks).
 *   tq_search_one  = tq_submit + tq_wait: the blocking, thread-safe single-query call.
 * A query the device does not take fails alone (TQ_ERR_*; tq_last_error on the waiting thread), its
 * batch mates are re-run without it. */
typedef struct tq_ticket tq_ticket;
int tq_submit(tq_segment *seg, const tq_query *query, const tq_search_opts *opts, float *out_scores,
              uint32_t *out_docs, uint32_t *out_count, tq_ticket **out);
int tq_wait(tq_ticket *ticket);
int tq_search_one(tq_segment *seg, const tq_query *query, const tq_search_opts *opts,
                  float *out_scores, uint32_t *out_docs, uint32_t *out_count);
typedef struct tq_submit_stats {
  uint64_t batches;   /* launches issued for submitted queries */
  uint64_t queries;   /* queries they carried */
  uint64_t max_batch; /* the largest of them */
} tq_submit_stats;
int tq_get_submit_stats(tq_segment *seg, tq_submit_stats *out, int reset);

/* replaces: TopBySortKeyCollector::merge_fruits -> merge_top_k
 * (src/collector/sort_key_top_collector.rs:54-95; ordering top_score_collector.rs:590-600):
 * merges n_segments per-segment results (layout [segment][query][stride], as gathered by an
 * all-gather over ranks) into the global top-(offset+limit) by (score desc, segment_ord asc,
 * doc asc), then skips `offset`.  Host version. */
int tq_merge_topk(const float *scores, const uint32_t *docs, const uint32_t *counts,
                  uint32_t n_segments, uint32_t n_queries, uint32_t stride, uint32_t offset,
                  uint32_t limit, float *out_scores, uint32_t *out_segment_ords,
                  uint32_t *out_docs, uint32_t *out_counts);
/* Device version of the same merge (inputs/outputs are device pointers on `device`; enqueued on
 * hip_stream).  segment_ords[s] gives the segment ordinal of slab s (NULL => s). */
int tq_merge_topk_device(tq_ctx *ctx, int device, const float *d_scores, const uint32_t *d_docs,
                         const uint32_t *d_counts, const uint32_t *segment_ords,
                         uint32_t n_segments, uint32_t n_queries, uint32_t stride,
                         uint32_t offset, uint32_t limit, float *d_out_scores,
                         uint32_t *d_out_segment_ords, uint32_t *d_out_docs,
                         uint32_t *d_out_counts, void *hip_stream);
/* The merged rows' way back to the host: an asynchronous copy of `bytes` from device memory on `device` to PINNED host
 * memory, enqueued on hip_stream behind the merge.  replaces: nothing in the reference (its fruits are host vectors);
 * what a Rust host does with hipMemcpyAsync after tq_merge_topk_device. */
int tq_copy_to_host_async(tq_ctx *ctx, int device, void *dst_pinned_host, const void *src_device, size_t bytes,
                          void *hip_stream);

/* ---- cross-GPU exchange (one segment set per GPU) ----
 * replaces: the fan-in of Searcher::search_with_executor (src/core/searcher.rs:230-235: the
 * executor maps collect_segment over the segments, src/core/executor.rs:61-104, and hands the
 * fruits to merge_fruits, src/collector/sort_key_top_collector.rs:54-95) when the segments live
 * on different GPUs, one process per GPU.  The only collective of the path: an RCCL all-gather of
 * the per-segment top-k lists over xGMI.  BM25 statistics need none (sums known to the host
 * before dispatch, src/query/bm25.rs:27-50).
 *
 * tq_comm_unique_id : ncclGetUniqueId on ONE rank; the host sends the 128 bytes to the others
 *                     (any channel: the Rust host's own control plane).
 * tq_comm_init      : ncclCommInitRank(world, id, rank) on `device`; collective over all ranks.
 * tq_allgather_topk : every rank passes the [n_rows][stride] result slabs of its local segments
 *                     (n_rows = local segments x queries; scores / docs, and [n_rows] counts) as
 *                     written by tq_search_batch_device, and receives all ranks' slabs as
 *                     [world][n_rows][stride] / [world][n_rows] — with rank r holding segments
 *                     r*S..r*S+S-1 that is the [segment][query][stride] input of
 *                     tq_merge_topk_device.  Device pointers; enqueued on hip_stream (stream
 *                     ordered after the searches, no host synchronisation); one grouped RCCL
 *                     launch.  librccl is opened at run time (TQ_RCCL_LIB overrides the path);
 *                     TQ_ERR_UNSUPPORTED if it cannot be loaded. */
#define TQ_COMM_ID_BYTES 128
typedef struct tq_comm tq_comm;
int tq_comm_unique_id(uint8_t *id_out /* TQ_COMM_ID_BYTES */);
int tq_comm_init(tq_ctx *ctx, int device, const uint8_t *id, int rank, int world, tq_comm **out);
void tq_comm_free(tq_comm *comm);
int tq_comm_info(const tq_comm *comm, int *rank, int *world, const char **library);
int tq_allgather_topk(tq_comm *comm, const float *d_scores, const uint32_t *d_docs,
                      const uint32_t *d_counts, uint32_t n_rows, uint32_t stride,
                      float *d_all_scores, uint32_t *d_all_docs, uint32_t *d_all_counts,
                      void *hip_stream);

/* ---- codec access (parity tests / tooling) ----
 * replaces: BlockSegmentPostings::load_block over a whole list (block_segment_postings.rs:343-391;
 * BitPacker4x decode + strict-delta prefix sum + vint tail).  docs/tfs: doc_freq u32 each (host). */
int tq_decode_postings(tq_segment *seg, tq_term_handle term, uint32_t *docs, uint32_t *tfs);
/* replaces: PositionReader::read over the whole term (positions/reader.rs:104-148): raw position
 * deltas, n_positions values (host); *n_out = number available. */
int tq_decode_position_deltas(tq_segment *seg, tq_term_handle term, uint32_t *out, uint64_t cap,
                              uint64_t *n_out);

/* ---- derived tables, read back (DIAGNOSTIC: tests of term preparation; no query path uses them) ----
 * replaces: nothing in the reference — the tables are this library's own (tq_device.h), built when a term is prepared.
 * tq_term_table_read copies ONE table of a prepared list, or of the segment, to the host as the device holds it: the
 * segment's stream is waited for, list maxima still on their way from tq_term_prepare_batch are applied, then plain
 * device-to-host copies — no kernel is launched and no device memory allocated.  *n_bytes = the table's size; a table
 * the list does not have: *n_bytes = 0 and TQ_OK.  out NULL or cap_bytes 0: the size alone; cap_bytes below the size,
 * an unknown `which`, a handle that is out of range or a released term set: TQ_ERR_INVALID.  Per-segment tables ignore
 * `term`.  Layouts: tantivy_amd/csrc/tq_device.h (TqdTermHead / TqdTerm / TqdSegment); TQ_TABLE_RMAX = every level as
 * laid out by tqd_rm_level_off; TQ_TABLE_RDIR = the directory words (padded to four), then one entry per posting;
 * TQ_TABLE_FLAT = the doc ids (padded to 16 bytes), then min(tf, 255) per posting; TQ_TABLE_LNORM = 128 bytes per block; TQ_TABLE_LMAT = 128 u64 per block, empty while the table is older than the doc matrix. */
enum {
  TQ_TABLE_REC = 0,        /* (n_blocks + 1) x 4 u32 */
  TQ_TABLE_COARSE = 1,
  TQ_TABLE_TAIL_DOCS = 2,
  TQ_TABLE_TAIL_TFS = 3,
  TQ_TABLE_POS_BLK = 4,
  TQ_TABLE_POS_TAIL = 5,
  TQ_TABLE_DENSE = 6,      /* {doc bits, rank} per 32 docs */
  TQ_TABLE_BITS = 7,
  TQ_TABLE_POS_DIR = 8,
  TQ_TABLE_TF8 = 9,
  TQ_TABLE_RMAX = 10,
  TQ_TABLE_RDIR = 11,
  TQ_TABLE_LNORM = 12,
  TQ_TABLE_FLAT = 13,
  TQ_TABLE_PROBE_DENSE = 14,   /* the probe pool's, while the list holds a slot */
  TQ_TABLE_PROBE_TF8 = 15,
  TQ_TABLE_PROBE_POS_DIR = 16,
  TQ_TABLE_LMAT = 17,          /* n_blocks x 128 u64: the doc-matrix words of the list's docs in posting order (empty while stale) */
  TQ_TABLE_DOCMAT = 32,        /* per segment: max_doc u64 */
  TQ_TABLE_DOCCLS = 33,        /* max_doc u64 */
  TQ_TABLE_LOCAL_CACHE = 34,   /* 256 floats: Bm25Weight.cache under the segment's own average fieldnorm */
  TQ_TABLE_MIN_FIELDNORM_ID = 35 /* one u32 */
};
typedef struct tq_term_table_info_t {
  uint32_t n_blocks, n_full, n_tail, coarse_shift;
  uint64_t payload_base;
  uint32_t has_freq;      /* TqdTermHead::has_freq: column slot, signature bit, tf-class flag, ... */
  uint32_t rdir_shift;    /* 0: no range directory */
  uint32_t rmax_list;     /* 255: none */
  uint32_t n_pos_blocks, n_pos_tail;
  uint32_t field;
  uint64_t n_positions;
  uint32_t doc_freq;
  uint32_t probe_slot;    /* 0xFFFFFFFF: the list holds no slot of the probe pool */
} tq_term_table_info_t;
int tq_term_table_read(tq_segment *seg, tq_term_handle term, uint32_t which, void *out, uint64_t cap_bytes,
                       uint64_t *n_bytes);
int tq_term_table_info(tq_segment *seg, tq_term_handle term, tq_term_table_info_t *info);

/* ---- codec writers (segment finalisation / merges on the device) ----
 * replaces: PostingsSerializer::{new_term, write_doc, close_term} (src/postings/serializer.rs:
 * 342-481; skip entries src/postings/skip.rs:55-88; block-max selection serializer.rs:404-428)
 * for a batch of terms.  Term t owns docs/tfs[term_starts[t] .. term_starts[t+1]) (doc ids
 * strictly increasing, tfs >= 1; tfs ignored / may be NULL with TQ_BASIC).  fieldnorm_ids =
 * num_docs bytes of the field's fieldnorm sub-file or NULL (then no block-max metadata, as when
 * the serializer has no FieldNormReader); avg_fieldnorm = total_num_tokens / num_docs
 * (serializer.rs:130-135).  Writes the posting lists back to back, exactly the bytes the
 * reference writes after the 8-byte total_num_tokens header of the field's .idx sub-file;
 * out_term_starts[t] .. [t+1] is TermInfo::postings_range relative to that point;
 * *out_len = bytes needed (valid also when TQ_ERR_INVALID reports out_cap too small). */
typedef struct tq_encoder tq_encoder;
int tq_encoder_create(tq_ctx *ctx, int device, tq_encoder **out);
void tq_encoder_free(tq_encoder *enc);
int tq_encode_postings(tq_encoder *enc, uint32_t n_terms, const uint64_t *term_starts,
                       const uint32_t *docs, const uint32_t *tfs, const uint8_t *fieldnorm_ids,
                       uint32_t num_docs, float avg_fieldnorm, uint8_t record_option, uint8_t *out,
                       uint64_t out_cap, uint64_t *out_term_starts, uint64_t *out_len);
/* replaces: PositionSerializer::{write_positions_delta, close_term} (src/positions/serializer.rs:
 * 46-91) for a batch of terms: term t owns position_deltas[term_starts[t] .. term_starts[t+1])
 * (the within-document deltas of all its docs, concatenated); output = the terms' .pos bytes back
 * to back, out_term_starts = TermInfo::positions_range. */
int tq_encode_positions(tq_encoder *enc, uint32_t n_terms, const uint64_t *term_starts,
                        const uint32_t *position_deltas, uint8_t *out, uint64_t out_cap,
                        uint64_t *out_term_starts, uint64_t *out_len);
/* Same with inputs and outputs resident in device memory (d_*); term_starts is needed on both
 * sides (host copy: block planning).  Only the 8-byte total crosses back to the host. */
int tq_encode_postings_device(tq_encoder *enc, uint32_t n_terms, const uint64_t *term_starts,
                              const uint64_t *d_term_starts, const uint32_t *d_docs,
                              const uint32_t *d_tfs, const uint8_t *d_fieldnorm_ids,
                              uint32_t num_docs, float avg_fieldnorm, uint8_t record_option,
                              uint8_t *d_out, uint64_t out_cap, uint64_t *d_out_term_starts,
                              uint64_t *out_len, void *hip_stream);
int tq_encode_positions_device(tq_encoder *enc, uint32_t n_terms, const uint64_t *term_starts,
                               const uint64_t *d_term_starts, const uint32_t *d_position_deltas,
                               uint8_t *d_out, uint64_t out_cap, uint64_t *d_out_term_starts,
                               uint64_t *out_len, void *hip_stream);
/* HIP-event time of the last call's kernels (measure + scan + write), milliseconds. */
int tq_encoder_last_kernel_ms(tq_encoder *enc, float *ms);

/* ---- deletes and counting ----
 * replaces: SegmentReader::alive_bitset + AliveBitSet::is_alive in the collector callback
 * (src/fastfield/alive_bitset.rs:52-61, src/collector/sort_key/sort_by_score.rs:44-53).  bytes =
 * the segment's `.del` file body as BitSet::serialize writes it (common/src/bitset.rs:215-223:
 * u32 LE max_value == max_doc, then 64-bit words); NULL = no deletes.  Deleted docs are skipped
 * by every search and count on this segment; BM25 statistics still count them, like the
 * reference (bm25.rs:38-45). */
int tq_segment_set_alive_bitset(tq_segment *seg, const uint8_t *bytes, size_t len);
/* replaces: Count collector (src/collector/count_collector.rs:39-80) over the same query shapes:
 * out_counts[q] = number of alive docs matching query q on this segment (the top-k fields of the
 * queries are ignored).  Host buffer. */
int tq_count_batch(tq_segment *seg, const tq_query *queries, uint32_t n_queries,
                   uint32_t *out_counts);
/* Number of docs scored per query by the last tq_search_batch* call on this segment (with
 * "exhaustive" = 1 that is the number of matches, which makes (Count, TopDocs) one pass). */
int tq_last_batch_match_counts(tq_segment *seg, uint32_t *out, uint32_t n_queries);
/* Per query of the last tq_search_batch* / tq_docset_batch* / tq_count_batch call on this segment: the candidate docs of
 * a sloppy phrase whose carried position list went over TQ_SLOP_CARRY_CAP (0 for every other query, and for every
 * query when the batch held no sloppy phrase), under the CALLER's query indices whatever sub-batches the call ran
 * internally; n_queries at most the queries of that call.  Waits for the batch like tq_last_batch_match_counts.
 * Non-zero = that query's rows / count are not to be trusted.  After a host-output call returned TQ_ERR_UNSUPPORTED for an
 * overflow the words stay readable: the error names the first such query, these words every one. */
int tq_last_batch_slop_overflows(tq_segment *seg, uint32_t *out, uint32_t n_queries);

/* ---- doc sets ----
 * replaces: Weight::for_each_no_score -> SegmentCollector::collect_block with the alive filter of
 * default_collect_segment_impl (src/query/weight.rs:23-35,101-121, src/query/boolean_query/boolean_weight.rs:536-560,
 * src/query/term_query/term_weight.rs:88-116, src/collector/mod.rs:186-221) — what DocSetCollector
 * (src/collector/docset_collector.rs:26-57), FilterCollector, facets and aggregations ask a Weight for: for every
 * query the ALIVE matching docs of this segment, ascending, back to back (CSR): query q owns
 * out_docs[out_starts[q] .. out_starts[q+1]).  out_starts has n_queries + 1 entries and is always filled when the
 * queries are valid; out_starts[n_queries] = total docs.  If that exceeds out_cap the call returns TQ_ERR_INVALID, has
 * written no doc at or past out_cap (the host variant: no doc at all), and the caller retries with a buffer of
 * out_starts[n_queries] entries (the protocol of tq_encode_postings' *out_len).  The top-k fields, weights and tf_cache
 * of the queries are ignored (weights / tf_cache may be NULL).
 * Query shapes: TQ_MODE_AND, TQ_MODE_OR and flat TQ_MODE_BOOL — occurs, clause_of unions, MustNot,
 * min_should_match "at least m of n Should clauses" for any m (a clause = the OR of the lists that share a clause_of
 * value and counts once; a clause without a list does not count toward n; m > n is the empty set) — with
 * TQ_TERM_ABSENT terms.  Every list is read as bitmap words (8 bytes per list per 32 docs; a list without a bitmap is
 * scattered into batch scratch first, see "docset_temp_lists"), twice: a count pass, a device prefix sum, a write pass.
 * Not taken: TQ_MODE_PHRASE and nested queries (tq_query.nested_occurs / atom_of trees) — a batch that holds one fails
 * as a whole with TQ_ERR_UNSUPPORTED, tq_last_error() names the index of the first such query, nothing is launched and
 * the segment stays usable; malformed queries (mixed occurs in one clause, occur > 2, handle out of range, n_terms 0
 * or > TQ_MAX_TERMS) return TQ_ERR_INVALID the same way.  Scores (Weight::for_each): tq_docset_scored_batch below.
 * With the option "docset_trees" = 1 both variants TAKE those shapes: TQ_MODE_PHRASE (phrase_offsets required), phrases
 * as boolean clauses and nested queries — whatever tq_search_batch takes as a tree: 2..8 terms per phrase, a field with
 * positions, minimums <= 15; weights may still be NULL.  A TQ_TERM_ALL clause inside a nested query, and whatever else
 * the tree planner refuses, fails the batch as above with the planner's code.  Every list of such a query is reached
 * through a bitmap (its own tables or the probe pool's, built on first use as for TQ_KERNEL_TREE; "use_dense" off:
 * TQ_ERR_UNSUPPORTED).  Cost: ONE result bitmap of batch scratch per such query (max_doc / 8 bytes, counted against
 * "docset_temp_lists" like a scattered list), written by docset_tree_bits_kernel — the tree's bitwise expression over
 * the lists' words, a phrase decided per candidate doc by walking its positions to the first place where the terms line
 * up — in front of the count pass, which then reads the query as one list.  kernel_mask gains TQ_KERNEL_DOCSET_TREE
 * when a query of the call took that kernel, and such a query adds (lists + 2) x bitmap words x 4 to algorithmic_bytes
 * (every list's bits once, the result word written and read back; positions are not counted) in place of lists x
 * bitmap words x 4.  tq_count_batch keeps its routes, and the scored calls below do not look at this option: they have
 * one of their own, "docset_score_trees".
 * Afterwards tq_last_batch_match_counts gives the per-query sizes, tq_batch_stats.matches the total docs,
 * kernel_mask = TQ_KERNEL_DOCSET and algorithmic_bytes = lists x bitmap words x 4 + 4 x docs. */
int tq_docset_batch(tq_segment *seg, const tq_query *queries, uint32_t n_queries,
                    uint32_t *out_docs, uint64_t out_cap, uint64_t *out_starts);
/* Same with DEVICE outputs on the segment's device, enqueued on hip_stream (NULL = the segment's stream), no
 * host synchronisation: docs whose position is >= out_cap are not written; d_out_starts[n_queries] tells the
 * consumer the total.  Returns TQ_OK even when the total exceeds out_cap (only the device knows). */
int tq_docset_batch_device(tq_segment *seg, const tq_query *queries, uint32_t n_queries,
                           uint32_t *d_out_docs, uint64_t out_cap, uint64_t *d_out_starts, void *hip_stream);

/* ---- doc sets with scores ----
 * replaces: Weight::for_each -> for_each_scorer (src/query/weight.rs:9-18,89-97) under default_collect_segment_impl
 * (src/collector/mod.rs:186-221) — what every collector whose requires_scoring() is true asks a Weight for
 * (TopDocs::tweak_score / custom_score, a MultiCollector with a scoring child, a user collector that reads the score):
 * every ALIVE matching doc with its BM25 score, however many there are (top-k stops at TQ_MAX_K).
 * out_docs / out_starts are exactly what tq_docset_batch returns for the same queries — same flat query shapes, same
 * refusals (by default TQ_MODE_PHRASE and nested queries: TQ_ERR_UNSUPPORTED naming the first such query, nothing launched —
 * also with "docset_trees" = 1, which only concerns the unscored calls; "docset_score_trees" = 1, which only concerns
 * the scored calls, takes them: below), same
 * capacity protocol — and out_scores[i] is the score of out_docs[i]; one out_cap covers both arrays (host variant, total
 * > out_cap: TQ_ERR_INVALID, out_starts complete, no doc and no score written).  Unlike tq_docset_batch, weights and
 * tf_cache are REQUIRED for every query that has a scoring (non-MustNot, present) list — TQ_ERR_INVALID naming the
 * query otherwise — and are used as in tq_search_batch; k is still ignored.
 * Scores are the unpruned scorers': per list bm25(weights[i], tf_cache[fieldnorm id], tf) with an IEEE divide (a
 * TQ_BASIC list scores tf = 1; no fieldnorms: the constant id); TQ_MODE_OR: 0 + the lists that hold the doc in query
 * order (SumCombiner); TQ_MODE_AND and the Must part of TQ_MODE_BOOL: clauses sorted by cost (stable), first + second
 * + (0 + the others) (Intersection::score, src/query/intersection.rs:325-329) — Should clauses that
 * min_should_match == n_should >= 2 turned into Must clauses join the sort; a clause of several lists scores the sum
 * of its present lists in clause order; Should clauses beside a Must part add req + opt with opt = the sum of the present
 * Should clauses (src/query/reqopt_scorer.rs:85-98).  One lane computes one doc's score in that order: the result does
 * not depend on the batch, the sub-batching or the run.
 * A scoring pass (tq_docset_score.hip) follows every write pass: it reads the rows back and asks each scoring list
 * for the doc's tf — through its bitmap + rank directory and byte-wide tfs, its range directory, or a block search.
 * Afterwards tq_last_batch_match_counts / tq_batch_stats.matches as for doc sets, kernel_mask = TQ_KERNEL_DOCSET |
 * TQ_KERNEL_DOCSET_SCORE, and algorithmic_bytes = the doc-set figure (lists x bitmap words x 4 + 4 x docs) + per doc
 * 4 (score) + 1 (fieldnorm byte) + per scoring list of every query 8 bytes per 32 docs of the segment (a bitmap word
 * with its rank: the most a list's presence and posting index cost; tf bytes are not counted).
 * With the option "docset_score_trees" = 1 both variants TAKE what the unscored calls take under "docset_trees" = 1:
 * TQ_MODE_PHRASE (phrase_offsets required), phrases as boolean clauses and nested queries, within the tree planner's
 * limits (2..8 terms per phrase, a field with positions, minimums <= 15).  The two options are independent.  weights and
 * tf_cache are REQUIRED for such a query (NULL, or a weight that is not finite: TQ_ERR_INVALID naming the query) and mean
 * what they mean to tq_search_batch: every term carries its own weight, each term of a phrase atom the phrase's weight,
 * a plain TQ_MODE_PHRASE query its weight in weights[0].  What the tree planner refuses — a negative boost inside a
 * nested query, a TQ_TERM_ALL clause inside a tree, a phrase on a field without positions, "use_dense" off — fails the
 * whole batch before any launch with the planner's code and "query N"; the segment stays usable.
 * The rows of such a query are written as for the unscored call (docset_tree_bits_kernel, then the count / scan / write
 * passes) and scored by docset_tree_score_kernel behind the write pass, one lane per doc over the planner's record:
 * tree_kernel's per-doc scoring stage — bitmap word, rank, tf byte (255: the packed tf of the posting's block); a phrase
 * atom scores bm25(its weight, norm, number of aligned positions) from the full cursor walk; sums in Intersection::score
 * / RequiredOptionalScorer / SumCombiner order, a Should clause only where it matches — so a doc scores bit for bit
 * what tq_search_batch's TQ_KERNEL_TREE gives it.  The flat scoring pass writes nothing over such a row.
 * kernel_mask of a scored call that held such a query: TQ_KERNEL_DOCSET | TQ_KERNEL_DOCSET_SCORE |
 * TQ_KERNEL_DOCSET_TREE | TQ_KERNEL_DOCSET_TREE_SCORE (flat queries only: the two bits above, whatever the option's
 * value).  Such a query adds to algorithmic_bytes the unscored tree figure, (lists + 2) x bitmap words x 4, per output
 * doc 4 (doc) + 4 (score) + 1 (fieldnorm), and per non-MustNot list of the tree (under a MustNot on neither level) 8
 * bytes per 32 docs of the segment; positions are not counted.  matches / tq_last_batch_match_counts as for the
 * unscored call. */
int tq_docset_scored_batch(tq_segment *seg, const tq_query *queries, uint32_t n_queries,
                           uint32_t *out_docs, float *out_scores, uint64_t out_cap, uint64_t *out_starts);
/* Same with DEVICE outputs, enqueued on hip_stream (NULL = the segment's stream): nothing is written at or past
 * out_cap in either array, the call returns TQ_OK and d_out_starts[n_queries] holds the total. */
int tq_docset_scored_batch_device(tq_segment *seg, const tq_query *queries, uint32_t n_queries,
                                  uint32_t *d_out_docs, float *d_out_scores, uint64_t out_cap,
                                  uint64_t *d_out_starts, void *hip_stream);

/* ---- sort by fast field ----
 * replaces: TopDocs::with_limit(k).order_by_fast_field(field, order) / order_by_u64_field / order_by((SortByStaticFastValue,
 * ComparatorEnum)) on one segment (src/collector/top_score_collector.rs:217-223,299-330; collect_segment_top_k,
 * src/collector/sort_key/sort_key_computer.rs:118-135): no scoring, the alive filter, and a TopNComputer over
 * Option<u64> = Column<u64>::first(doc) (sort_by_static_fast_value.rs:62-96).  Row q holds the first min(k, matches) alive
 * matching docs of query q under compare_for_top_k: the comparator on the key, then ASCENDING doc id whatever the order.
 * The four ComparatorEnum values are two choices (order.rs:68-221,286-293):
 *   Natural (= Order::Desc)            TQ_SORT_DESC, TQ_NULLS_LAST
 *   ReverseNoneLower (= Order::Asc)    TQ_SORT_ASC,  TQ_NULLS_LAST
 *   Reverse                            TQ_SORT_ASC,  TQ_NULLS_FIRST
 *   NaturalNoneHigher                  TQ_SORT_DESC, TQ_NULLS_FIRST
 * Docs without a value (a TQ_CARD_OPTIONAL column) are never dropped: they tie with each other, in doc order, after or
 * before every doc with a value.  `column` is a handle of tq_column_upload (multivalued columns cannot be uploaded, so
 * first(doc) is the doc's only value).
 * tq_query.k is the query's offset+limit, 1..TQ_MAX_K; weights, tf_cache and the pruning fields are ignored (may be NULL).
 * Outputs: row q = entries [q * out_stride, (q + 1) * out_stride) of out_docs / out_values / out_has_value, in result
 * order, out_stride >= the largest k; out_values is in the column's u64 space (the caller applies T::from_u64, as the
 * reference does after the top-k) and 0 where out_has_value is 0; the padding behind out_counts[q] real entries is
 * (TQ_TERMINATED, 0, 0).  Nothing is written at or past a row's out_stride.
 * Query shapes: exactly what tq_docset_batch takes under the segment's current options — flat AND / OR / BOOL with
 * clause_of, MustNot and m-of-n, TQ_TERM_ALL, term-set and range handles as lists; under "docset_trees" = 1 also phrases,
 * sloppy phrases and nested queries — with tq_docset_batch's refusals, codes and "query N" text under this function's
 * name: the whole batch fails before any launch and the segment stays usable.  TQ_ERR_INVALID with a message: a column
 * index out of range or a released column, order or nulls above 1, k of 0 or above TQ_MAX_K, out_stride below the largest k.
 * No doc set is written: after the doc-set path's scatter / tree / sloppy-phrase launches, one selection launch per
 * sub-batch (tq_sort.hip: workgroup = (query, slice of the bitmap words); match bits, column decode and a wavefront
 * top-k over 98-bit keys (class, value or its complement, ~doc)) and, with more than one slice per query (option
 * "sort_slices"), a merge launch.
 * Afterwards tq_last_batch_match_counts gives every query's number of alive matches (Count + TopDocs in one pass),
 * tq_batch_stats.matches their sum, kernel_mask = TQ_KERNEL_SORT (| TQ_KERNEL_DOCSET_TREE | TQ_KERNEL_PHRASE_SLOP where such
 * a query ran), and
 *   algorithmic_bytes = the doc-set figure for reading every list's words ONCE (lists x bitmap words x 4; a tree:
 *                       (lists + 2) x bitmap words x 4)
 *                     + 8 per matching doc with a value
 *                     + 8 per matching doc of a TQ_CARD_OPTIONAL column (its presence word)
 *                     + 13 per row entry written (doc, value, flag). */
enum tq_sort_order { TQ_SORT_DESC = 0, TQ_SORT_ASC = 1 };
enum tq_sort_nulls { TQ_NULLS_LAST = 0, TQ_NULLS_FIRST = 1 };
int tq_search_sorted_batch(tq_segment *seg, const tq_query *queries, uint32_t n_queries,
                           uint32_t column, uint8_t order, uint8_t nulls, uint32_t out_stride,
                           uint32_t *out_docs, uint64_t *out_values, uint8_t *out_has_value, uint32_t *out_counts);
/* Same with DEVICE outputs on the segment's device, enqueued on hip_stream (NULL = the segment's stream), no host
 * synchronisation: returns TQ_OK once the work is enqueued, like tq_search_batch_device. */
int tq_search_sorted_batch_device(tq_segment *seg, const tq_query *queries, uint32_t n_queries,
                                  uint32_t column, uint8_t order, uint8_t nulls, uint32_t out_stride,
                                  uint32_t *d_out_docs, uint64_t *d_out_values, uint8_t *d_out_has_value,
                                  uint32_t *d_out_counts, void *hip_stream);

/* ---- aggregations over a fast field: stats and histogram ----
 * replaces, on one segment and for every query of a batch: a `stats` metric (count / sum / min / max / avg:
 * src/aggregation/metric/stats.rs:86-176, IntermediateStats::collect and finalize) and optionally a `histogram` bucket
 * aggregation — which with nanosecond arguments is also `date_histogram` with a fixed_interval — over a resident u64
 * column (src/aggregation/bucket/histogram/histogram.rs:468-518 collect, :672-699 normalize_histogram_req, :738-769
 * get_bucket_pos_f64 and compute_dense_range; src/aggregation/mod.rs:351-383 f64_from_fastfield_u64; common/src/lib.rs:
 * 108-114 u64_to_f64), over the query's ALIVE MATCHING docs, in one pass over its match bits: no doc set is written.
 *
 * Value types: TQ_VALUE_U64 (also Bool), TQ_VALUE_I64 (also DateTime, nanoseconds), TQ_VALUE_F64 — how the column's u64
 * space maps back (MonotonicallyMappableToU64).
 *
 * Stats, one tq_agg_stats_t per query:
 *   matches               alive matching docs            count        those with a value (a TQ_CARD_OPTIONAL column)
 *   min_value, max_value  in the column's U64 SPACE; UINT64_MAX / 0 when count == 0.  The three mappings keep order, so the
 *                         caller converts after the fact, as for out_values of the sorted call
 *   sum_lo, sum_hi        the exact 128-bit sum of the u64-space values.  U64: the sum.  I64: subtract count * 2^63.  The
 *                         reference adds f64 with Kahan's algorithm in doc order; the integer sum is exact and order-free
 *                         and equals it wherever every partial sum is below 2^53.  TQ_VALUE_F64: a sum in u64 space means
 *                         nothing — both words are WRITTEN AS 0 (F64 sums are not served)
 *   in_bounds             docs with a value inside the histogram's bounds = the sum of the row (0 without a histogram)
 *   out_of_range          docs inside the bounds whose bucket fell outside the row: always 0 (see below), never written
 * NaNs of an F64 column sit at the two ends of the mapped order, so min_value / max_value can be a NaN where the
 * reference's f64::min / f64::max skip NaNs: not emulated.
 *
 * Histogram (histogram != 0).  Per doc with a value: val = f64_from_fastfield_u64(value) — U64 (double)v, I64
 * (double)(int64_t)(v ^ 1 << 63), F64 from_bits(v & 1 << 63 ? v ^ 1 << 63 : ~v); if bounds_min <= val && val <= bounds_max
 * the doc counts in bucket pos = (int64)floor((val - offset) / interval), the cast saturating.  The bounds are the hard
 * bounds, or (-DBL_MAX, DBL_MAX) without them — the test is always made, so +-inf and NaN are never counted — and hard
 * bounds that cannot exclude a value of the column (col min >= hard_min && col max <= hard_max) collapse to that
 * sentinel.  Rows are DENSE over compute_dense_range: lo = max(f(col min), bounds_min), hi = min(f(col max), bounds_max),
 * nothing when lo > hi (or the column has no row), base_pos = pos(lo), n_buckets = pos(hi) - base_pos + 1; entry i of a
 * row is bucket base_pos + i, whose key is (base_pos + i) * interval + offset.  Subtraction, division by a positive
 * interval and floor are monotonic, so every counted doc falls inside the row; the kernel still checks.  All of it is
 * IEEE double arithmetic without contraction: device, host and any model agree bit for bit.  Date columns: interval,
 * offset and bounds in nanoseconds (normalize_date_time applied by the caller).  Keys, gap filling, extended_bounds,
 * min_doc_count, keyed and ordering are the caller's post-processing.
 *
 * tq_agg_histogram_plan is the host-only part (no device, like tq_column_parse): validation and the dense range, from a
 * column's tq_column_info_t.  n_buckets == 0 when no value can be in bounds.  TQ_ERR_INVALID: interval <= 0 or not
 * finite, offset not finite, hard bounds not finite or hard_min > hard_max, value_type above TQ_VALUE_F64.
 * TQ_ERR_UNSUPPORTED naming the count: more than TQ_AGG_MAX_BUCKETS buckets (the reference's DEFAULT_BUCKET_LIMIT of 65 000
 * rounded up to a power of two).  With histogram == 0 only value_type is checked and the plan is empty.
 *
 * tq_agg_batch: host outputs, blocking.  Buckets are uint32_t (a segment has fewer than 2^31 docs); row q = out_buckets +
 * q * bucket_stride, of which entries [0, n_buckets) are written and NOTHING else; bucket_stride < n_buckets is
 * TQ_ERR_INVALID; out_buckets may be NULL when histogram == 0 (or n_buckets == 0).  tq_query.k is ignored; weights,
 * tf_cache and the pruning fields too.  Query shapes, options ("docset_trees", "docset_temp_lists"), refusals, codes and
 * "query N" texts are tq_docset_batch's under this function's name, as for tq_search_sorted_batch; a column index out of
 * range or a released column, and what the plan refuses, fail the whole batch before any launch and leave the segment
 * usable.  A sloppy phrase whose carried list went over the cap: TQ_ERR_UNSUPPORTED naming it after the rows are written,
 * as for tq_search_sorted_batch (the device variant: tq_last_batch_slop_overflows).
 * Launches: after the doc-set path's scatter / tree / sloppy-phrase launches, one that initialises the records and rows
 * and one aggregation launch per sub-batch (tq_agg.hip: workgroup = (query, slice of the bitmap words), option
 * "agg_slices"; per-lane accumulators, wavefront shuffles, and integer vector atomics on the query's record and row — order-
 * free, hence deterministic; a histogram of at most "agg_lds_buckets" buckets is counted in LDS first).
 * Afterwards tq_last_batch_match_counts gives `matches`, kernel_mask = TQ_KERNEL_AGG (| TQ_KERNEL_DOCSET_TREE |
 * TQ_KERNEL_PHRASE_SLOP), and
 *   algorithmic_bytes = lists x bitmap words x 4 (a tree: (lists + 2) x bitmap words x 4)
 *                     + 8 per matching doc with a value
 *                     + 8 per matching doc of a TQ_CARD_OPTIONAL column (its presence word)
 *                     + (64 + 4 x n_buckets) per query. */
enum tq_value_type { TQ_VALUE_U64 = 0, TQ_VALUE_I64 = 1, TQ_VALUE_F64 = 2 };
#define TQ_AGG_MAX_BUCKETS 65536u
typedef struct tq_agg_request {
  uint32_t column;         /* handle of tq_column_upload */
  uint8_t value_type;      /* tq_value_type */
  uint8_t histogram;       /* 0: stats alone; 1: and the histogram below */
  uint8_t has_hard_bounds; /* 0 / 1 */
  uint8_t reserved;
  double interval, offset;
  double hard_min, hard_max;
} tq_agg_request; /* 40 bytes */
typedef struct tq_agg_hist_plan_t {
  int64_t base_pos;   /* bucket of a row's entry 0 */
  uint32_t n_buckets; /* 0: no value can be in bounds */
  uint32_t reserved;
  double bounds_min, bounds_max; /* the effective bounds: hard, or the (-DBL_MAX, DBL_MAX) sentinel */
} tq_agg_hist_plan_t; /* 32 bytes */
typedef struct tq_agg_stats_t {
  uint64_t matches, count;
  uint64_t min_value, max_value;
  uint64_t sum_lo, sum_hi;
  uint64_t in_bounds, out_of_range;
} tq_agg_stats_t; /* 64 bytes */
int tq_agg_histogram_plan(const tq_column_info_t *info, const tq_agg_request *req, tq_agg_hist_plan_t *out);
int tq_agg_batch(tq_segment *seg, const tq_query *queries, uint32_t n_queries, const tq_agg_request *req,
                 tq_agg_stats_t *out_stats, uint32_t *out_buckets, uint32_t bucket_stride);
/* Same with DEVICE outputs on the segment's device, enqueued on hip_stream (NULL = the segment's stream), no host
 * synchronisation.  The call itself zeroes what it accumulates into: the same buffers may be used again. */
int tq_agg_batch_device(tq_segment *seg, const tq_query *queries, uint32_t n_queries, const tq_agg_request *req,
                        tq_agg_stats_t *d_out_stats, uint32_t *d_out_buckets, uint32_t bucket_stride, void *hip_stream);

/* ---- sub-aggregations: stats of a second column per histogram bucket ----
 * replaces a `histogram` / `date_histogram` with ONE `stats` / `avg` / `min` / `max` / `sum` / `value_count` sub-aggregation
 * (src/aggregation/bucket/histogram/histogram.rs:489-505, the nested path of collect; src/aggregation/metric/stats.rs:
 * 282-306 SegmentStatsCollector::collect under a parent_bucket_id, :164 IntermediateStats::collect): "avg / max of latency
 * per hour".  One pass over every query's match bits, no doc set written.
 *
 * req is tq_agg_batch's request for the BUCKET column A and must ask for the histogram (histogram == 0: TQ_ERR_INVALID); the
 * plan is tq_agg_histogram_plan's.  out_stats and out_buckets are what tq_agg_batch writes for the same request, bit for bit.
 * out_bucket_stats: row q = out_bucket_stats + q * bucket_stride — the count rows' stride — of which entries [0, n_buckets)
 * are written and NOTHING else; entry i is the record of the METRIC column B over exactly the docs counted in bucket i
 * (the docs with a value in A inside the effective bounds; a doc outside them, or without a value in A, enters no record):
 *   count                 those docs with a value in B (a TQ_CARD_OPTIONAL B without a value contributes nothing: the
 *                         reference's fetch_block_with_missing with missing = None)
 *   min_value, max_value  in B's u64 space; UINT64_MAX / 0 when count == 0
 *   sum_lo, sum_hi        the exact 128-bit sum of B's u64-space values, as in tq_agg_stats_t (it equals the reference's
 *                         Kahan f64 sum in doc order wherever every partial sum is below 2^53)
 * B has its own value type: with TQ_VALUE_F64 both sum words are written as 0 and min / max can be a NaN at either end of
 * the mapped order.  B may be the column A.
 * Refused before any launch, the segment stays usable (TQ_ERR_INVALID): what tq_agg_batch refuses, histogram == 0, a metric
 * column that is not live, a metric value_type above TQ_VALUE_F64, a null out_bucket_stats when n_buckets > 0.  Query
 * shapes, options, the sloppy-phrase verdict and the message texts are tq_agg_batch's under this function's name.
 * Launches: tq_agg_batch's, with the records initialised beside the rows and agg_sub_kernel (tq_agg_sub.hip) as the
 * aggregation launch: per bucketed doc a second column read, then the bucket's entry of a workgroup-private LDS table
 * (n_buckets <= min("agg_lds_buckets", the kernel's capacity: 40 bytes per bucket) — flushed once with vector atomics) or,
 * above it, the query's row and records directly.  Integer atomics: deterministic.
 * Afterwards tq_last_batch_match_counts as before, kernel_mask = TQ_KERNEL_AGG_SUB (| TQ_KERNEL_DOCSET_TREE |
 * TQ_KERNEL_PHRASE_SLOP), and
 *   algorithmic_bytes = tq_agg_batch's for column A
 *                     + 8 per bucketed doc with a value in B
 *                     + 8 per bucketed doc of a TQ_CARD_OPTIONAL B (its presence word)
 *                     + 40 x n_buckets per query.
 * Not served: several metric columns or sibling aggregations in one call, nested buckets, `missing`, F64 sums. */
typedef struct tq_agg_metric_request {
  uint32_t column;     /* metric column B: a handle of tq_column_upload; may equal req->column */
  uint8_t value_type;  /* tq_value_type of B */
  uint8_t reserved[3]; /* zero */
} tq_agg_metric_request; /* 8 bytes */
typedef struct tq_agg_bucket_stats_t {
  uint64_t count;                /* docs of the bucket with a value in B */
  uint64_t min_value, max_value; /* B's u64 space; UINT64_MAX / 0 when count == 0 */
  uint64_t sum_lo, sum_hi;       /* exact 128-bit sum; TQ_VALUE_F64: written as 0 */
} tq_agg_bucket_stats_t; /* 40 bytes */
int tq_agg_sub_batch(tq_segment *seg, const tq_query *queries, uint32_t n_queries, const tq_agg_request *req,
                     const tq_agg_metric_request *metric, tq_agg_stats_t *out_stats, uint32_t *out_buckets,
                     tq_agg_bucket_stats_t *out_bucket_stats, uint32_t bucket_stride);
/* Same with DEVICE outputs, enqueued on hip_stream (NULL = the segment's stream), no host synchronisation.  The call itself
 * zeroes what it accumulates into: the same buffers may be used again. */
int tq_agg_sub_batch_device(tq_segment *seg, const tq_query *queries, uint32_t n_queries, const tq_agg_request *req,
                            const tq_agg_metric_request *metric, tq_agg_stats_t *d_out_stats, uint32_t *d_out_buckets,
                            tq_agg_bucket_stats_t *d_out_bucket_stats, uint32_t bucket_stride, void *hip_stream);
/* The LDS tables' capacities in buckets of the two instantiations of agg_sub_kernel: out[0] the small one, out[1] the
 * large one; a histogram of more than min("agg_lds_buckets", out[1]) buckets is accumulated in global memory. */
void tq_agg_sub_lds_capacities(uint32_t out[2]);

/* ---- terms aggregation: the top values of a fast field by doc count ----
 * replaces a `terms` bucket aggregation over a resident u64 column ("top 10 status among +body:error +timestamp:[a TO b]";
 * src/aggregation/bucket/term_agg/mod.rs:836-899 SegmentTermCollector::collect, :1000-1111
 * into_intermediate_bucket_result, :1328-1353 cut_off_buckets, :316-335 TermsAggregationInternal::from_req), per query of
 * a batch, in one pass over the query's match bits and one selection pass on the device: no doc set is written and only
 * the surviving (key, doc_count) pairs leave the device.
 *
 * Per query, over its alive matching docs that have a value in the column (TQ_CARD_FULL or TQ_CARD_OPTIONAL; a doc without
 * a value enters nothing: `missing` is not served): a value's key index is (value - min_value) / gcd, an exact integer in
 * [0, n_keys), n_keys = (max_value - min_value) / gcd + 1 — no f64 anywhere, so keys above 2^53 are exact.  The ENTRIES
 * are the indices with a doc count > 0, ordered by req->order:
 *   TQ_TERMS_COUNT_DESC   count descending, ties by ascending key (the reference's default order)
 *   TQ_TERMS_COUNT_ASC    count ascending, ties by ascending key
 *   TQ_TERMS_KEY_ASC      key ascending
 *   TQ_TERMS_KEY_DESC     key descending
 * (the reference cuts with select_nth_unstable / sort_unstable: which of several equal-count keys survive at the cut is
 * unspecified there; here it is the ascending key, always).  The first n_returned = min(segment_size, distinct) entries are
 * written in that order: out_keys[q * out_stride + j] = min_value + gcd * index — the column's u64 space: a term ordinal of
 * a str / bytes column, which the caller resolves in the dictionary; I64 / F64 / Date are mapped back as out_values of
 * tq_search_sorted_batch — and out_counts[q * out_stride + j] its doc count.  One tq_agg_terms_t per query:
 *   matches                      alive matching docs
 *   count                        those with a value = the sum of all entries' counts
 *   sum_other_doc_count          the sum of the counts from entry number segment_size on (cut_off_buckets)
 *   distinct                     entries before the cut
 *   n_returned                   entries written
 *   doc_count_error_upper_bound  the count of entry number segment_size (0-based) in that order, 0 if there is none
 *   out_of_range                 docs whose index fell outside [0, n_keys): 0 by the column's own min / max / gcd
 * sum_other_doc_count and doc_count_error_upper_bound do not depend on the tie-break.  `size`, `min_doc_count`,
 * `show_term_doc_count_error`, the merge across segments and the final cut are the caller's post-processing; segment_size
 * is the reference's (default 10 x size).
 *
 * tq_agg_terms_plan is the host-only part (no device): n_keys, min_value and gcd from a column's tq_column_info_t, and the
 * validation of the request.  A column without a row plans n_keys = 0: the call then returns records of zeros with
 * `matches` filled.  TQ_ERR_UNSUPPORTED naming n_keys: more than TQ_AGG_MAX_BUCKETS keys (the count rows are dense, sized
 * like the histogram's; the reference's hash-map path for high-cardinality columns is not served).  TQ_ERR_INVALID:
 * segment_size == 0 or > TQ_AGG_TERMS_MAX_SIZE (tq_agg_terms_max_size), an order above TQ_TERMS_KEY_DESC.
 *
 * tq_agg_terms_batch: host outputs, blocking.  Of row q entries [0, n_returned) hold the result; the host variant writes
 * entries [n_returned, min(segment_size, n_keys)) as zeros and nothing past them.  Refused before any launch, the segment
 * stays usable: what the plan refuses, a column that is not live, out_stride < min(segment_size, n_keys), null outputs
 * (TQ_ERR_INVALID).  Query shapes, options ("agg_slices", "agg_lds_buckets", "docset_trees", "docset_temp_lists"), the
 * sloppy-phrase verdict and the message texts are tq_agg_batch's under this function's name.
 * Launches: after the doc-set path's scatter / tree / sloppy-phrase launches, one that initialises the records and the
 * per-query count rows — n_queries x n_keys x 4 bytes of segment scratch, never an output —, one agg_terms_count_kernel
 * launch per sub-batch (tq_agg_terms.hip: agg_kernel's walk; counts in a workgroup-private LDS table when n_keys <=
 * min("agg_lds_buckets", tq_agg_terms_lds_capacities' large capacity), else vector atomics on the scratch row) and ONE
 * agg_terms_select_kernel launch behind the last sub-batch (a workgroup per query: radix select of the cut, compaction, a
 * sort in LDS).  Integer arithmetic only: deterministic.
 * Afterwards tq_last_batch_match_counts gives `matches`, kernel_mask = TQ_KERNEL_AGG_TERMS (| TQ_KERNEL_DOCSET_TREE |
 * TQ_KERNEL_PHRASE_SLOP), and
 *   algorithmic_bytes = lists x bitmap words x 4 (a tree: (lists + 2) x bitmap words x 4)
 *                     + 8 per matching doc with a value
 *                     + 8 per matching doc of a TQ_CARD_OPTIONAL column (its presence word)
 *                     + (40 + 4 x n_keys) per query + 12 per entry returned.
 * Not served here: a sub-aggregation under terms and ordering by it (tq_agg_terms_sub_batch below), `missing`, `include` / `exclude`, multivalued columns,
 * more than TQ_AGG_MAX_BUCKETS keys. */
#define TQ_AGG_TERMS_MAX_SIZE 1024u
enum tq_terms_order { TQ_TERMS_COUNT_DESC = 0, TQ_TERMS_COUNT_ASC = 1, TQ_TERMS_KEY_ASC = 2, TQ_TERMS_KEY_DESC = 3 };
typedef struct tq_agg_terms_request {
  uint32_t column;       /* handle of tq_column_upload */
  uint32_t order;        /* tq_terms_order */
  uint32_t segment_size; /* 1 .. TQ_AGG_TERMS_MAX_SIZE */
} tq_agg_terms_request; /* 12 bytes */
typedef struct tq_agg_terms_plan_t {
  uint64_t min_value, gcd; /* key = min_value + gcd * index */
  uint32_t n_keys;         /* 0: the column has no row */
  uint32_t reserved;
} tq_agg_terms_plan_t; /* 24 bytes */
typedef struct tq_agg_terms_t {
  uint64_t matches, count;
  uint64_t sum_other_doc_count;
  uint32_t distinct, n_returned;
  uint32_t doc_count_error_upper_bound, out_of_range;
} tq_agg_terms_t; /* 40 bytes */
int tq_agg_terms_plan(const tq_column_info_t *info, const tq_agg_terms_request *req, tq_agg_terms_plan_t *out);
int tq_agg_terms_batch(tq_segment *seg, const tq_query *queries, uint32_t n_queries, const tq_agg_terms_request *req,
                       tq_agg_terms_t *out_terms, uint64_t *out_keys, uint32_t *out_counts, uint32_t out_stride);
/* Same with DEVICE outputs, enqueued on hip_stream (NULL = the segment's stream), no host synchronisation.  Entries at or
 * past n_returned of a row are NOT touched.  The call itself zeroes what it accumulates into: the same buffers may be used
 * again. */
int tq_agg_terms_batch_device(tq_segment *seg, const tq_query *queries, uint32_t n_queries, const tq_agg_terms_request *req,
                              tq_agg_terms_t *d_out_terms, uint64_t *d_out_keys, uint32_t *d_out_counts, uint32_t out_stride,
                              void *hip_stream);
/* The LDS tables' capacities in keys of the two instantiations of agg_terms_count_kernel: out[0] the small one, out[1] the
 * large one; more than min("agg_lds_buckets", out[1]) keys are counted in global memory. */
void tq_agg_terms_lds_capacities(uint32_t out[2]);
uint32_t tq_agg_terms_max_size(void); /* TQ_AGG_TERMS_MAX_SIZE */

/* ---- terms aggregation with a metric: stats of a second column per key, and order by it ----
 * replaces a `terms` aggregation with ONE stats / avg / min / max / sum / value_count sub-aggregation, optionally ordered
 * by it ("top 10 service by avg latency among +body:error +timestamp:[a TO b]", `"order": {"lat.avg": "desc"}`;
 * src/aggregation/bucket/term_agg/mod.rs:836-899 collect with a sub-aggregation, :1040-1111 the order by a
 * sub-aggregation and cut_off_buckets; src/aggregation/metric/stats.rs:282-306, :325-357 compute_metric_value).
 *
 * Per query, over its alive matching docs that have a value in the key column A — exactly what tq_agg_terms_batch runs
 * over, with its plan (tq_agg_terms_plan) and its exact integer key index: each key gets a doc count and a
 * tq_agg_bucket_stats_t over the docs counted under it: `count` the number of those docs that have a value in the metric
 * column B (which may be A), min_value / max_value in B's u64 space (UINT64_MAX / 0 when count == 0), the exact 128-bit
 * sum (TQ_VALUE_F64: both sum words 0, as for tq_agg_sub_batch).  The entries are the keys with a doc count > 0; the first
 * min(segment_size, distinct) are written in req->order as (out_keys, out_counts, out_entry_stats)[q * out_stride + j].
 * The tq_agg_terms_t record means what it means for tq_agg_terms_batch: the error bound is the doc count of entry number
 * segment_size in the order used, sum_other_doc_count the doc counts from that entry on — cut_off_buckets, which the
 * reference also applies under a sub-aggregation order.
 *
 * Orders: the four of tq_agg_terms_batch — record, keys and counts are then that call's, bit for bit — and
 *   TQ_TERMS_METRIC_DESC  the largest order value first, ties by ascending key
 *   TQ_TERMS_METRIC_ASC   the smallest order value first, ties by ascending key
 * (the reference's select_nth_unstable_by(partial_cmp) leaves ties unspecified).  The ORDER VALUE of an entry is a
 * fixed-width unsigned integer image of req->order_metric of its record, monotone in the typed value, the one
 * tq_agg_terms_metric_image returns (the same code the kernel runs):
 *   TQ_METRIC_VALUE_COUNT  the record's count
 *   TQ_METRIC_MIN / _MAX   the u64-space value (tantivy's mapping is monotone for U64 / I64 / F64)
 *   TQ_METRIC_SUM          the exact typed sum as a biased 96-bit integer: U64 the sum; I64 sum - count x 2^63 + 2^95
 *   TQ_METRIC_AVG          the monotone u64 image (f64_to_u64) of the f64 that is the CORRECTLY ROUNDED (half to even)
 *                          quotient of the exact typed sum by count — integer long division, not f64 arithmetic on a
 *                          rounded sum
 * An entry whose record has count == 0 orders as typed 0 under MIN / MAX / AVG (compute_metric_value(..).unwrap_or(0.0)).
 * The exact order refines the reference's f64 order: it can only separate what f64 ties.
 *
 * Refused before any launch, the segment stays usable, the message carries the called function's name: everything
 * tq_agg_terms_batch refuses; TQ_ERR_INVALID: an order above TQ_TERMS_METRIC_ASC, an order_metric above TQ_METRIC_AVG
 * under a metric order, non-zero reserved, a metric column that is not live, a metric_value_type above TQ_VALUE_F64, a null
 * out_entry_stats when min(segment_size, n_keys) > 0; TQ_ERR_UNSUPPORTED naming the pair: a SUM or AVG order over a
 * TQ_VALUE_F64 metric (F64 sums are not served).  Query shapes, options, the sloppy-phrase verdict and the message texts
 * are tq_agg_batch's under this function's name.
 * Launches: after the doc-set path's launches one that initialises the records and the scratch — per query a count row and a
 * record row, n_keys x 44 bytes of segment scratch, never an output —, one agg_terms_sub_count_kernel launch per sub-batch
 * (tq_agg_terms_sub.hip; a workgroup-private LDS table when n_keys <= min("agg_lds_buckets",
 * tq_agg_terms_sub_lds_capacities' large capacity), else vector atomics on the scratch rows) and ONE
 * agg_terms_sub_select_kernel launch behind the last sub-batch.  Integer arithmetic only: deterministic.
 * Afterwards kernel_mask = TQ_KERNEL_AGG_TERMS_SUB (| TQ_KERNEL_DOCSET_TREE | TQ_KERNEL_PHRASE_SLOP), and
 *   algorithmic_bytes = tq_agg_terms_batch's
 *                     + 8 per counted doc with a value in B
 *                     + 8 per counted doc of a TQ_CARD_OPTIONAL B (its presence word)
 *                     + 40 x n_keys per query + 40 per entry returned.
 * Not served: more than one metric column, nested bucket aggregations, `missing`, `include` / `exclude`, F64 sums,
 * multivalued columns, more than TQ_AGG_MAX_BUCKETS keys. */
/* two more values of tq_terms_order, for tq_agg_terms_sub_batch* alone (tq_agg_terms_plan / tq_agg_terms_batch* refuse them) */
#define TQ_TERMS_METRIC_DESC 4u
#define TQ_TERMS_METRIC_ASC 5u
enum tq_terms_metric { TQ_METRIC_VALUE_COUNT = 0, TQ_METRIC_MIN = 1, TQ_METRIC_MAX = 2, TQ_METRIC_SUM = 3, TQ_METRIC_AVG = 4 };
typedef struct tq_agg_terms_sub_request {
  uint32_t column;            /* key column A */
  uint32_t order;             /* tq_terms_order, 0..5 */
  uint32_t segment_size;      /* 1 .. TQ_AGG_TERMS_MAX_SIZE */
  uint32_t metric_column;     /* metric column B (may be A) */
  uint8_t metric_value_type;  /* tq_value_type of B */
  uint8_t order_metric;       /* tq_terms_metric; read only under the two METRIC orders */
  uint8_t reserved[2];        /* zero */
} tq_agg_terms_sub_request; /* 20 bytes */
int tq_agg_terms_sub_batch(tq_segment *seg, const tq_query *queries, uint32_t n_queries, const tq_agg_terms_sub_request *req,
                           tq_agg_terms_t *out_terms, uint64_t *out_keys, uint32_t *out_counts,
                           tq_agg_bucket_stats_t *out_entry_stats, uint32_t out_stride);
/* Same with DEVICE outputs, enqueued on hip_stream (NULL = the segment's stream), no host synchronisation.  Entries at or
 * past n_returned of a row are NOT touched. */
int tq_agg_terms_sub_batch_device(tq_segment *seg, const tq_query *queries, uint32_t n_queries, const tq_agg_terms_sub_request *req,
                                  tq_agg_terms_t *d_out_terms, uint64_t *d_out_keys, uint32_t *d_out_counts,
                                  tq_agg_bucket_stats_t *d_out_entry_stats, uint32_t out_stride, void *hip_stream);
/* The LDS tables' capacities in keys of the two instantiations of agg_terms_sub_count_kernel: out[0] the small one, out[1]
 * the large one; more than min("agg_lds_buckets", out[1]) keys are accumulated in global memory. */
void tq_agg_terms_sub_lds_capacities(uint32_t out[2]);
/* The order value of one record (host only, no device): out[0] the low 64 bits, out[1] the high ones (non-zero for
 * TQ_METRIC_SUM alone).  TQ_ERR_INVALID: a null argument, a value_type above TQ_VALUE_F64, a metric above TQ_METRIC_AVG, a
 * count of 2^32 or more or a sum of 2^96 or more; TQ_ERR_UNSUPPORTED: SUM or AVG of TQ_VALUE_F64. */
int tq_agg_terms_metric_image(const tq_agg_bucket_stats_t *rec, uint32_t value_type, uint32_t metric, uint64_t out[2]);

/* ---- range aggregation: doc counts and a metric column's stats per range of a fast field ----
 * replaces a `range` bucket aggregation over a resident u64 column, alone or with ONE stats / avg / min / max / sum /
 * value_count sub-aggregation ("how many of +body:error per latency band <10 / 10-100 / 100-1000 / >=1000 ms, and the avg of
 * bytes in each"; src/aggregation/bucket/range.rs:276-305 collect, :431-437 get_bucket_pos, :451-473 to_u64_range, :477-519
 * extend_validate_ranges; src/aggregation/mod.rs:394-402 f64_to_fastfield_u64).  One pass over every query's match bits,
 * no doc set written, no f64 on the device: the request's bounds are converted into the column's u64 space once, on the
 * host, and u64 values are compared.
 *
 * tq_agg_range_plan is the host-only part (no device): the request's ranges as BUCKETS [start, end) of the u64 space, in
 * bucket order.  A bound converts as the reference's `as` casts do, saturating: TQ_VALUE_U64 (also Bool) negatives -> 0,
 * >= 2^64 -> UINT64_MAX, else truncated; TQ_VALUE_I64 (also DateTime, nanoseconds) saturated to i64, then ^ 1 << 63;
 * TQ_VALUE_F64 the monotone image of its bits; no `from`: 0, no `to`: UINT64_MAX.  Then extend_validate_ranges: a stable
 * sort by start, a bucket [0, first start) in front unless the first start is 0, a bucket [last end, UINT64_MAX) behind
 * unless the last end is UINT64_MAX, every hole between neighbours filled.  `source` of a bucket is the index of the
 * caller's range it came from (custom keys stay the caller's, found through it), UINT32_MAX for an inserted bucket.
 * out_buckets holds `cap` entries; *out_n_buckets is written whenever the plan exists, also when cap is too small.
 * TQ_ERR_INVALID, in this order: a null argument, n_ranges == 0 (the reference indexes [0] and panics), value_type above
 * TQ_VALUE_F64, non-zero reserved bytes, a NaN bound, a range whose converted start is above its converted end (named; the
 * reference takes it and then searches a list that is no longer sorted), neighbours that overlap — end > next start — (both
 * named), cap below the plan's buckets.  TQ_ERR_UNSUPPORTED naming the count: more than TQ_AGG_RANGE_MAX_BUCKETS buckets.
 *
 * A value falls into THE LAST BUCKET WHOSE START IS <= THE VALUE (tq_agg_range_bucket_of: the code the kernel runs, a
 * branch-free search whose trip count depends on n alone).  For strictly increasing starts that is the reference's
 * binary_search_by_key(..).unwrap_or_else(|p| p - 1); UINT64_MAX falls into the last bucket, as in the reference's release
 * build.  An EMPTY range (start == end after conversion: 0.1 .. 0.2 on an integer column) shares its start with its
 * successor and counts nothing — what [s, s) contains; the reference's count there depends on which of the equal elements
 * its binary search happens to meet.
 *
 * tq_agg_range_batch: host outputs, blocking.  metric == NULL: doc counts alone.
 *   out_stats         one tq_agg_stats_t per query, tq_agg_batch's record of column A bit for bit; in_bounds == count (every
 *                     doc with a value has a bucket), out_of_range always 0
 *   out_counts        row q = out_counts + q * bucket_stride: entry i = the alive matching docs with a value in A in bucket i
 *   out_bucket_stats  with a metric alone; row q = out_bucket_stats + q * bucket_stride: entry i = the record of the metric
 *                     column B over exactly the docs counted in bucket i, by tq_agg_sub_batch's rule (count = those with a
 *                     value in B, min / max in B's u64 space, the exact 128-bit sum; TQ_VALUE_F64: both sum words 0).  B may
 *                     be A
 * Entries [0, n_buckets) of a row are written and NOTHING else.  Integer atomics only: the same call gives the same bytes.
 * Refused before any launch, the segment stays usable: what the plan refuses; TQ_ERR_INVALID for a column that is not live,
 * a metric column that is not live, a metric value_type above TQ_VALUE_F64 or non-zero reserved bytes of it, bucket_stride
 * < n_buckets, a null out_counts, a null out_bucket_stats with a metric.  Query shapes, options ("docset_trees",
 * "docset_temp_lists", "agg_slices", "agg_lds_buckets"), sub-batches, the sloppy-phrase verdict and the "query N" texts are
 * tq_agg_batch's under this function's name.
 * Launches: tq_agg_batch's (tq_agg_sub_batch's with a metric) with agg_range_kernel (tq_agg_range.hip) as the aggregation
 * launch; in front of them the starts go up through a pinned staging buffer, once per call, and every workgroup copies
 * them into LDS.  Counts alone: a uint32_t LDS table when n_buckets <= "agg_lds_buckets", else atomics on the query's row.
 * With a metric: the 40-byte LDS table when n_buckets <= min("agg_lds_buckets", tq_agg_range_lds_capacities' large
 * capacity), else the query's row and records.
 * Afterwards tq_last_batch_match_counts gives `matches`, kernel_mask = TQ_KERNEL_AGG_RANGE (| TQ_KERNEL_DOCSET_TREE |
 * TQ_KERNEL_PHRASE_SLOP), and
 *   algorithmic_bytes = tq_agg_batch's for column A with this n_buckets
 *                     + 8 x n_buckets per call (the starts)
 *                     + with a metric: 8 per bucketed doc with a value in B
 *                                    + 8 per bucketed doc of a TQ_CARD_OPTIONAL B (its presence word)
 *                                    + 40 x n_buckets per query.
 * Not served: several metric columns, sibling or nested bucket aggregations, `keyed`, DateTime key formatting (keys are the
 * caller's), `missing`, F64 sums, multivalued columns, more than TQ_AGG_RANGE_MAX_BUCKETS buckets. */
#define TQ_AGG_RANGE_MAX_BUCKETS 1024u
typedef struct tq_agg_range_t {
  double from, to;         /* read when has_from / has_to; the column's typed space (DateTime: nanoseconds) */
  uint8_t has_from, has_to; /* 0 / 1 */
  uint8_t reserved[6];     /* zero */
} tq_agg_range_t; /* 24 bytes */
typedef struct tq_agg_range_request {
  uint32_t column;     /* bucket column A: a handle of tq_column_upload (tq_agg_range_plan does not read it) */
  uint8_t value_type;  /* tq_value_type of A */
  uint8_t reserved[3]; /* zero */
  uint32_t n_ranges;
  uint32_t reserved2;  /* zero */
  const tq_agg_range_t *ranges;
} tq_agg_range_request; /* 24 bytes */
typedef struct tq_agg_range_bucket_t {
  uint64_t start, end; /* [start, end) in the column's u64 space */
  uint32_t source;     /* index into the request's ranges; UINT32_MAX: inserted by the plan */
  uint32_t reserved;
} tq_agg_range_bucket_t; /* 24 bytes */
int tq_agg_range_plan(const tq_agg_range_request *req, tq_agg_range_bucket_t *out_buckets, uint32_t cap, uint32_t *out_n_buckets);
/* The bucket of `value` among n buckets with these starts (non-decreasing, starts[0] == 0): the last start <= value.  Host
 * only; starts == NULL or n == 0: 0. */
uint32_t tq_agg_range_bucket_of(const uint64_t *starts, uint32_t n, uint64_t value);
int tq_agg_range_batch(tq_segment *seg, const tq_query *queries, uint32_t n_queries, const tq_agg_range_request *req,
                       const tq_agg_metric_request *metric, tq_agg_stats_t *out_stats, uint32_t *out_counts,
                       tq_agg_bucket_stats_t *out_bucket_stats, uint32_t bucket_stride);
/* Same with DEVICE outputs, enqueued on hip_stream (NULL = the segment's stream), no host synchronisation.  The call itself
 * zeroes what it accumulates into: the same buffers may be used again. */
int tq_agg_range_batch_device(tq_segment *seg, const tq_query *queries, uint32_t n_queries, const tq_agg_range_request *req,
                              const tq_agg_metric_request *metric, tq_agg_stats_t *d_out_stats, uint32_t *d_out_counts,
                              tq_agg_bucket_stats_t *d_out_bucket_stats, uint32_t bucket_stride, void *hip_stream);
/* The 40-byte LDS tables' capacities in buckets of the two metric instantiations of agg_range_kernel: out[0] the small one,
 * out[1] the large one (1 024 records, 1 024 starts and the walk's slabs are exactly the static 64 KB); with a metric, more
 * than min("agg_lds_buckets", out[1]) buckets are accumulated in global memory.  Counts alone fit LDS up to
 * TQ_AGG_RANGE_MAX_BUCKETS. */
void tq_agg_range_lds_capacities(uint32_t out[2]);

/* ---- terms x histogram: a (date_)histogram per key of a terms aggregation ----
 * replaces a `terms` aggregation over a low-cardinality column T with ONE `histogram` / `date_histogram` leaf over a column
 * H below it ("requests per hour for each status among +body:error +timestamp:[a TO b]";
 * src/aggregation/bucket/term_agg/term_histogram.rs, the fused collector: a flat grid counts[term * num_time_buckets +
 * bucket] and per term the docs outside hard_bounds; the general buffered path gives the same result and defines the
 * Optional cases).  Per query of a batch, one pass over the query's match bits; no doc set is written and only the
 * surviving keys' rows leave the device.
 *
 * Per query, over its alive matching docs: a doc without a value in T enters nothing (it counts in `matches` alone).  A doc
 * with key index i = (value - min) / gcd of T counts once under key i — tq_agg_terms_batch's exact integer index, its plan
 * (tq_agg_terms_plan on T), its four orders with ties at the cut to the ascending key, its tq_agg_terms_t record with the
 * same meaning of every field, its out_keys / out_counts: record, keys and counts are that call's, bit for bit.  The doc is
 * counted in cell (i, b) when it has a value in H, that value as tq_agg_batch's f64 passes the plan's effective bounds, and
 * b = floor((val - offset) / interval) - base_pos: tq_agg_batch's arithmetic and tq_agg_histogram_plan's plan on H, hard
 * bounds that cannot exclude a value of H dropped.  Otherwise — no value in H, or out of bounds — it is counted in the
 * key's OUTSIDE entry.  A key's doc count is the sum of its cells plus its outside entry (the reference's in_bounds +
 * out_of_bounds).  H may be T.
 * For query q and returned entry j, in the order used: out_keys[q * out_stride + j], out_counts[q * out_stride + j], and the
 * key's dense histogram row out_hist[(q * out_stride + j) * hist_stride + b], b in [0, n_buckets); bucket b has the key
 * (base_pos + b) * interval + offset, as for tq_agg_batch.  The outside entry does not leave the device: it is the doc
 * count minus the row's sum.
 *
 * tq_agg_terms_hist_plan is the host-only part (no device): the terms plan of info_t, the histogram plan of info_h, and
 * n_cells = n_keys x (n_buckets + 1), the grid of one query — the + 1 is the outside entry, the last of each key's row, so
 * that one index serves every doc and a key's doc count is one row sum.  n_buckets == 0 (no value of H within bounds, or H
 * without a row) is served: every doc of a key goes to its outside entry, the keys come back with empty rows.  n_keys == 0
 * returns records of zeros with `matches`.  TQ_ERR_INVALID: a null argument, non-zero reserved fields (the request's, the
 * histogram half's), a histogram half with histogram != 1, what tq_agg_terms_plan and tq_agg_histogram_plan refuse;
 * TQ_ERR_UNSUPPORTED: what those two refuse so, and n_cells > TQ_AGG_MAX_BUCKETS, naming n_keys and n_buckets (four times
 * the reference's MAX_FUSED_GRID_BUCKETS: the dense scratch row tq_agg_terms_batch allows per query) — all under this
 * function's name.
 *
 * tq_agg_terms_hist_batch: host outputs, blocking.  Of the row set q entries [0, n_returned) hold the result; the host
 * variant writes entries [n_returned, min(segment_size, n_keys)) — keys, counts and their histogram rows' [0, n_buckets) —
 * as zeros and nothing past them.  Refused before any launch, the segment stays usable: what the plan refuses, a column
 * that is not live, out_stride < min(segment_size, n_keys), hist_stride < n_buckets, null outputs (TQ_ERR_INVALID).  Query
 * shapes, options ("agg_slices", "agg_lds_buckets", "docset_trees", "docset_temp_lists"), the sloppy-phrase verdict and the
 * message texts are tq_agg_batch's under this function's name.
 * Launches: after the doc-set path's scatter / tree / sloppy-phrase launches, one that initialises the records and the
 * scratch — per query a grid row of n_cells and a totals row of n_keys entries, n_queries x (n_cells + n_keys) x 4 bytes of
 * segment scratch, never an output —, one agg_terms_hist_count_kernel launch per sub-batch (tq_agg_terms_hist.hip: the
 * shared walk; per doc a read of T, a read of H, the f64 bucket arithmetic and one add on its cell — of a workgroup-private
 * LDS table when n_cells <= min("agg_lds_buckets", tq_agg_terms_hist_lds_capacities' large capacity), else of the query's
 * grid row) and, behind the last sub-batch, three: the row sums into the totals rows, agg_terms_select_kernel over them
 * (tq_agg_terms_batch's own selection), and a gather of the survivors' rows, a wavefront per returned entry.  Integer
 * arithmetic and integer vector atomics only: deterministic.
 * Afterwards tq_last_batch_match_counts gives `matches`, kernel_mask = TQ_KERNEL_AGG_TERMS_HIST (| TQ_KERNEL_DOCSET_TREE |
 * TQ_KERNEL_PHRASE_SLOP), and
 *   algorithmic_bytes = tq_agg_terms_batch's for column T
 *                     + 8 per counted doc with a value in H
 *                     + 8 per counted doc of a TQ_CARD_OPTIONAL H (its presence word)
 *                     + 4 x n_cells per query + 4 x n_buckets per entry returned.
 * Not served: a metric under the histogram, several leaves, `min_doc_count` / `extended_bounds` (the caller's
 * post-processing of dense rows), `missing`, multivalued columns, grids above TQ_AGG_MAX_BUCKETS cells. */
typedef struct tq_agg_terms_hist_request {
  tq_agg_terms_request terms; /* the key column T, the order, segment_size */
  uint32_t reserved;          /* zero */
  tq_agg_request hist;        /* the histogram column H: tq_agg_batch's request with histogram == 1 */
} tq_agg_terms_hist_request; /* 56 bytes */
typedef struct tq_agg_terms_hist_plan_t {
  tq_agg_terms_plan_t terms; /* tq_agg_terms_plan of T */
  tq_agg_hist_plan_t hist;   /* tq_agg_histogram_plan of H */
  uint32_t n_cells;          /* n_keys x (n_buckets + 1) <= TQ_AGG_MAX_BUCKETS */
  uint32_t reserved;
} tq_agg_terms_hist_plan_t; /* 64 bytes */
int tq_agg_terms_hist_plan(const tq_column_info_t *info_t, const tq_column_info_t *info_h, const tq_agg_terms_hist_request *req,
                           tq_agg_terms_hist_plan_t *out);
int tq_agg_terms_hist_batch(tq_segment *seg, const tq_query *queries, uint32_t n_queries, const tq_agg_terms_hist_request *req,
                            tq_agg_terms_t *out_terms, uint64_t *out_keys, uint32_t *out_counts, uint32_t *out_hist,
                            uint32_t out_stride, uint32_t hist_stride);
/* Same with DEVICE outputs, enqueued on hip_stream (NULL = the segment's stream), no host synchronisation.  Nothing at or
 * past n_returned of a row set — keys, counts, histogram rows — and nothing at or past n_buckets of a histogram row is
 * touched.  The call itself zeroes what it accumulates into: the same buffers may be used again. */
int tq_agg_terms_hist_batch_device(tq_segment *seg, const tq_query *queries, uint32_t n_queries,
                                   const tq_agg_terms_hist_request *req, tq_agg_terms_t *d_out_terms, uint64_t *d_out_keys,
                                   uint32_t *d_out_counts, uint32_t *d_out_hist, uint32_t out_stride, uint32_t hist_stride,
                                   void *hip_stream);
/* The LDS tables' capacities in cells of the two instantiations of agg_terms_hist_count_kernel: out[0] the small one, out[1]
 * the large one; a grid of more than min("agg_lds_buckets", out[1]) cells is counted in global memory. */
void tq_agg_terms_hist_lds_capacities(uint32_t out[2]);

/* ---- introspection ---- */
typedef struct tq_batch_stats {
  uint64_t algorithmic_bytes; /* sum len(postings_range) [+positions] + matches + 8k */
  uint64_t matches;           /* docs whose BM25 was evaluated (AND/phrase matches, OR union) */
  float kernel_ms;            /* HIP-event time of the scan kernel(s), mean over the batches */
  float total_ms;             /* ... of the whole batch on the stream: launched since the last call */
  uint32_t tiles;
  uint32_t chunks;
  uint32_t batches_averaged;  /* how many batches kernel_ms / total_ms average (<= 16) */
  float host_plan_ms;         /* host CPU time inside tq_search_batch_device (validate + plan + stage +
                                 enqueue; waiting for the previous batch's staging copy excluded),
                                 mean over the calls since the last tq_last_batch_stats */
  uint32_t kernel_mask;       /* TQ_KERNEL_*: the scan-kernel families the last batch was run by */
  uint64_t unique_bytes;      /* each DISTINCT posting list (+ positions, phrases) of the last batch once:
                                 what the batch needs from the index when no byte is read twice; the
                                 per-query sum above counts a list once per query that names it */
} tq_batch_stats;
/* scan-kernel families (tq_batch_stats.kernel_mask) */
#define TQ_KERNEL_AND_DENSE 0x001u    /* and_kernel, every non-leader list with a bitmap */
#define TQ_KERNEL_AND 0x002u          /* and_kernel, general */
#define TQ_KERNEL_UNION 0x004u        /* union_kernel (candidate-driven, per query) */
#define TQ_KERNEL_OR_WINDOWS 0x008u   /* or_kernel (4096-doc windows) */
#define TQ_KERNEL_PHRASE 0x010u       /* phrase_kernel */
#define TQ_KERNEL_PHRASE_SWEEP 0x020u /* phrase_sweep_kernel */
#define TQ_KERNEL_BOOL 0x040u         /* union_kernel, boolean instantiation */
#define TQ_KERNEL_USHARE 0x080u       /* ushare_kernel (unions, term-major for the batch) */
#define TQ_KERNEL_XUNION 0x100u       /* xunion_kernel (unpruned unions, doc-major for the batch) */
#define TQ_KERNEL_ASHARE 0x200u       /* ashare_kernel (intersections, leader-major for the batch) */
#define TQ_KERNEL_BSHARE 0x400u       /* ashare_kernel, boolean leads (TQ_MODE_BOOL, leader-major) */
#define TQ_KERNEL_COUNT_BITMAPS 0x800u /* count_bitmap_kernel (tq_count_batch over bitmap words) */
#define TQ_KERNEL_TREE 0x1000u         /* tree_kernel (nested boolean queries over bitmap words) */
#define TQ_KERNEL_DOCSET 0x2000u       /* docset_count / docset_write kernels (tq_docset_batch* over bitmap words) */
#define TQ_KERNEL_DOCSET_SCORE 0x4000u /* docset_score kernel (tq_docset_scored_batch*: the scoring pass behind the write pass) */
#define TQ_KERNEL_ALL 0x8000u          /* all_kernel (ALL-BASED queries: TQ_TERM_ALL clauses, over bitmap words) */
#define TQ_KERNEL_DOCSET_TREE 0x10000u /* docset_tree_bits_kernel (tq_docset_batch*, option "docset_trees": phrases and nested queries as match bits) */
#define TQ_KERNEL_DOCSET_TREE_SCORE 0x20000u /* docset_tree_score_kernel (tq_docset_scored_batch*, option "docset_score_trees": the scores of such rows) */
#define TQ_KERNEL_PHRASE_SLOP 0x40000u /* phrase_slop_kernel / phrase_slop_bits_kernel (TQ_MODE_PHRASE with slop > 0, over bitmap words) */
#define TQ_KERNEL_SORT 0x80000u        /* sort_select_kernel / sort_merge_kernel (tq_search_sorted_batch*: top k by a fast-field column) */
#define TQ_KERNEL_AGG 0x100000u        /* agg_kernel (tq_agg_batch*: stats and histogram of a fast-field column) */
#define TQ_KERNEL_AGG_SUB 0x200000u    /* agg_sub_kernel (tq_agg_sub_batch*: the histogram with a metric column's stats per bucket) */
#define TQ_KERNEL_AGG_TERMS 0x400000u  /* agg_terms_count_kernel / agg_terms_select_kernel (tq_agg_terms_batch*: the top values of a column by doc count) */
#define TQ_KERNEL_AGG_TERMS_SUB 0x800000u /* agg_terms_sub_count_kernel / agg_terms_sub_select_kernel (tq_agg_terms_sub_batch*: a metric column's stats per key, order by it) */
#define TQ_KERNEL_AGG_RANGE 0x1000000u /* agg_range_kernel (tq_agg_range_batch*: doc counts and a metric column's stats per range of a column) */
#define TQ_KERNEL_AGG_TERMS_HIST 0x2000000u /* agg_terms_hist_count_kernel / _rowsum_ / _gather_ (tq_agg_terms_hist_batch*: a histogram of a second column per key) */
int tq_last_batch_stats(tq_segment *seg, tq_batch_stats *out);
/* Which scan-kernel family (one TQ_KERNEL_* bit) evaluated every query of the last tq_search_batch* call on this
 * segment; needs the option "record_query_kernels" set before that call (diagnosis / parity tooling: bench.py
 * draws its oracle sample from every family a batch ran on). */
int tq_last_batch_query_kernels(tq_segment *seg, uint32_t *out, uint32_t n_queries);
/* Bytes the segment keeps resident in HBM, by kind: the reference's own sub-files (copied
 * verbatim) and the derived side tables of DESIGN.md section 2 — term tables (unrolled skip
 * records, coarse seek tables, decoded vint tails, position-block tables: what SkipReader /
 * PositionReader hold per open term in the reference), bitmaps + rank directories of the dense
 * lists, the doc matrix, position directories — plus the per-batch scratch. */
typedef struct tq_segment_stats {
  uint64_t index_bytes, positions_bytes, fieldnorm_bytes, alive_bytes; /* tantivy's bytes */
  uint64_t term_table_bytes, bitmap_bytes /* + byte-wide tfs */, docmat_bytes, posdir_bytes; /* derived */
  uint64_t scratch_bytes;       /* the segment's own batch scratch: staging, threshold slots, result slabs */
  uint64_t dense_budget_bytes;  /* cap on bitmap (+ byte-wide tf) + docmat + posdir bytes ("dense_budget_x") */
  uint32_t n_terms, n_dense_lists, n_docmat_columns;
  uint32_t probe_evictions;     /* lists whose probe tables ("probe_budget_x") gave their slot to another list */
  uint64_t device_scratch_bytes; /* partial / result lists + staging lists of the term-major launches: ONE set
                                    per device, shared by all its segments (count it once per device) */
  uint64_t lead_mat_bytes;      /* leaders' doc-matrix words in posting order ("lead_mat_budget_x"): derived, a budget of their own */
  uint32_t lead_mat_stale;      /* leaders of the last planned batch whose such table was older than the doc matrix: not used */
  uint32_t pad_;
} tq_segment_stats;
int tq_segment_get_stats(tq_segment *seg, tq_segment_stats *out);
/* knobs: "exhaustive" (0/1, default 0: block-max pruning as block_wand / block_wand_intersection
 *        do — the reference's execution; 1: score every match — same top-k either way, and
 *        tq_last_batch_match_counts then returns match counts),
 *        "timing" (0/1: record HIP events per batch),
 *        "dense" (0/1, default 1: tq_term_prepare also builds a bitmap + rank directory for lists
 *        with doc_freq >= max_doc/dense_ratio, while bitmaps + doc matrix + position directories
 *        stay below "dense_budget_x" times the segment's bytes), "dense_ratio" (default 128), "use_dense" (0/1, default 1: the AND kernel may use
 *        them),
 *        "or_windows" (-1/0/1, default -1 = auto: unions run window-parallel when exhaustive and
 *        candidate-driven when pruning; 0 / 1 force one kernel),
 *        "bound_slack_ppm" (default 0): block-max bounds are widened by (1 + ppm * 1e-6).  The
 *        block-max pairs were selected under the segment's own average fieldnorm
 *        (serializer.rs:130-135); a caller whose Bm25Weights use global statistics passes
 *        ((1 + d)^2 - 1) * 1e6 with d = relative difference of the two averages and pruning
 *        stays exact (the reference accepts the approximation, term_scorer.rs:58-70),
 *        "dense_budget_x" (default 8: bitmaps + byte-wide term freqs of the dense lists + doc matrix
 *        + doc signatures + position directories together stay below this multiple of the
 *        segment), "docmat" (0/1, default 1: the first 40 dense lists also get a column in a
 *        doc-major matrix: one 8-byte word per doc = fieldnorm id + the doc's membership in those
 *        lists), "docsig" (0/1, default 1: the top 16 bits of those words are a signature of the
 *        prepared lists WITHOUT a column: a clear bit proves the doc is not in such a list), "device_prepare" (0/1, default 0: tq_term_prepare
 *        works on the device copy even when a host copy exists; always so for segments from
 *        tq_segment_upload_device),
 *        "xunion_ratio" (default 64, 0 = never) / "xunion_min_queries" (default 64): with
 *        "exhaustive", pure unions (<= 8 lists, k <= 128, positive weights) whose lists together
 *        hold >= max_doc / xunion_ratio postings are evaluated doc-major for the whole batch —
 *        every list's tf/(tf+norm) built once per 128-doc tile, every query reading its lists' rows —
 *        when the batch has that many of them (up to 255 distinct lists and 8192 queries; lists
 *        without a bitmap are then also kept as plain doc / tf arrays, inside "dense_budget_x"),
 *        "probe_budget_x" (default 16, 0 = never): a boolean query rides in the shared leader-major launch
 *        (TQ_KERNEL_BSHARE) only if every list it probes has a bitmap + byte-wide tfs; for lists below
 *        "dense_ratio" they are built the first time a boolean query (or a nested one: TQ_KERNEL_TREE reaches EVERY
 *        list through a bitmap) names the list, into one of the equal slots of the segment's probe pool — this
 *        multiple of the segment's bytes worth of slots, at least TQ_MAX_TERMS; a list that needs a slot when all are
 *        taken gets the slot of the list used longest ago (tq_segment_stats.probe_evictions), never one the batch
 *        being planned uses: a batch that names more such lists than the budget holds grows the pool (the other
 *        kernels keep treating these lists as sparse),
 *        "rdir_budget_x" (default 4, 0 = never): tq_term_prepare / tq_term_prepare_batch also give a list below
 *        "dense_ratio" with at least 256 postings a RANGE DIRECTORY — one u32 per posting in posting order (16 bits of
 *        the doc id, min(tf, 0xFFFF)) and the number of postings before every 2^S-doc range, S chosen per list so
 *        that a range holds one to two postings: 6-8 bytes per posting, counted in
 *        tq_segment_stats.term_table_bytes — while the directories stay below this multiple of the segment's bytes.
 *        The shared intersection launch (TQ_KERNEL_ASHARE) probes the second list of a 2-term intersection through
 *        it ("is doc d in the list, with which tf": two directory slots and the range's entries) and drops the
 *        leader blocks in whose doc span the directory counts no posting; before, such a list needed a
 *        max_doc / 4-byte slot of the probe pool (19 x the segment's bytes resident after a 65 536-term stream,
 *        5 x with directories),
 *        "lead_mat_budget_x" (default 4, 0 = none built, none used) / "lead_mat_cut" (default 16): a list that leads
 *        queries of the shared intersection launch and holds at most max_doc / cut postings gets the doc-matrix words
 *        of its docs in posting order (8 bytes per posting, tq_segment_stats.lead_mat_bytes), while such tables stay
 *        below this multiple of the segment's bytes: the launch reads them as one 16-byte load per lane instead of
 *        two gathers.  A table is a copy: it is used only while no term was prepared since it was filled, and
 *        refilled once a batch finds the doc matrix unchanged since the batch before it,
 *        "count_bitmap_ratio" (default 128, 0 = never): tq_count_batch evaluates a query as a bitwise
 *        expression over bitmap words (4-8 bytes per list per 32 docs, no postings decoded; a list
 *        without a bitmap is scattered into a scratch bitmap once per batch) when the clause a scan
 *        would walk holds at least max_doc / ratio postings per list of the query,
 *        "docset_temp_lists" (default 0 = as many max_doc / 8-byte bitmaps as 1 GB — TQ_COUNT_TEMP_MB — holds, at most
 *        4096; never below TQ_MAX_TERMS, so a single query always fits): tq_docset_batch* — how many lists without a
 *        bitmap one launch scatters into batch scratch; a batch that names more of them runs as consecutive
 *        sub-batches of whole queries (out_starts continues across them; the caller sees one call),
 *        "docset_trees" (0/1, default 0; any other value: TQ_ERR_INVALID): tq_docset_batch / tq_docset_batch_device
 *        also take TQ_MODE_PHRASE, phrases as boolean clauses and nested queries (TQ_KERNEL_DOCSET_TREE; one scratch
 *        bitmap per such query, see "doc sets"); 0: they are refused with TQ_ERR_UNSUPPORTED as before.  The scored
 *        variants do not look at it,
 *        "docset_score_trees" (0/1, default 0; any other value: TQ_ERR_INVALID): tq_docset_scored_batch /
 *        tq_docset_scored_batch_device also take those shapes (TQ_KERNEL_DOCSET_TREE | TQ_KERNEL_DOCSET_TREE_SCORE; weights
 *        and tf_cache required, see "doc sets with scores"); 0: refused with TQ_ERR_UNSUPPORTED as before.  Independent
 *        of "docset_trees", which the unscored variants alone look at,
 *        "sort_slices" (0..256, default 0; any other value: TQ_ERR_INVALID): tq_search_sorted_batch* — slices of the
 *        segment's bitmap words per query, one selection workgroup each; 0 = the host chooses (queries x slices fills the
 *        machine, no slice below 1024 words), 1 = every query's row is written by its one workgroup and no merge is
 *        launched, 2..256 = forced (a slice past the last word is empty).  Results do not depend on it,
 *        "agg_slices" (0..256, default 0; any other value: TQ_ERR_INVALID): tq_agg_batch*, tq_agg_sub_batch*,
 *        tq_agg_terms_batch*, tq_agg_terms_sub_batch*, tq_agg_range_batch* — slices of the segment's
 *        bitmap words per query, one aggregation workgroup each; 0 = the host chooses as for "sort_slices", 1..256 =
 *        forced (a slice past the last word is empty).  Results do not depend on it,
 *        "agg_lds_buckets" (0..8192 = the kernel's LDS capacity, default 8192; any other value: TQ_ERR_INVALID):
 *        tq_agg_batch* — the largest n_buckets a workgroup counts in a private LDS table that it flushes once (a
 *        table of 2 048 buckets, or of 8 192 at half the wavefronts per SIMD: two instantiations); above it every doc is
 *        an atomic add on the query's row, several times slower on dense queries.  tq_agg_sub_batch*: min(the option,
 *        tq_agg_sub_lds_capacities' large capacity); tq_agg_terms_batch*: min(the option, tq_agg_terms_lds_capacities'
 *        large capacity) keys; tq_agg_terms_sub_batch*: min(the option, tq_agg_terms_sub_lds_capacities' large capacity)
 *        keys; tq_agg_range_batch*: the option for counts alone, min(the option, tq_agg_range_lds_capacities' large
 *        capacity) with a metric.  Results do not depend on it,
 *        "ashare_min_batch" (default 16; 512 until round 6): intersections take the shared leader-major launch
 *        (TQ_KERNEL_ASHARE) when at least this many queries of the batch qualify for it — below, its
 *        two launches and per-task set-up cost more than sharing the leader blocks saves (round 6, synchronous
 *        batches, shared against per-query: 8 queries 0.23 ms against 0.26; 16: 0.25 against 0.37; 64: 0.34
 *        against 0.44; 256: 0.64 against 0.69 — the batches concurrent single-query callers coalesce into),
 *        "ashare_inline_warm" (0 / 1 / 2, default 1; any other value: TQ_ERR_INVALID): the shared intersections' warm-up
 *        tasks (the first 2 permille of every leader's blocks, which leave the other tasks a threshold to start from)
 *        0 = in a dispatch of their own before the main one, 2 = in front of ONE dispatch, followed by the main tasks
 *        of leaders that have no warm-up task — as many as the resident wavefronts that find no warm-up task —, then by
 *        all the others in doc-slice order, 1 = as 2 where the intersections are the batch's only launch group and have
 *        that many independent tasks, else as 0 (a small batch keeps its barrier; next to another group's kernels the
 *        chip is not the launch's own).  Results do not depend on it: thresholds are advisory,
 *        "submit_window_us" (default 100): tq_submit / tq_search_one — how long the leader of a batch
 *        holds it open for the callers of the previous batch to come back with their next query
 *        (0 = launch with whatever is pending),
 *        "use_dpp" (0/1: DPP or ds_bpermute prefix sums),
 *        "record_query_kernels" (0/1, default 0: see tq_last_batch_query_kernels), "debug" (-1 = the TQ_DEBUG
 *        environment word, else the kernels' diagnosis word for this segment: work counters / ablations) */
int tq_set_option(tq_segment *seg, const char *name, int64_t value);

#ifdef __cplusplus
}
#endif
#endif
