// tq_docset_batch / tq_docset_batch_device: the full doc set of every query of a batch (Weight::for_each_no_score ->
// SegmentCollector::collect_block with the alive filter, src/query/weight.rs:23-35,101-121, src/collector/mod.rs:186-221)
// as CSR rows of ascending doc ids.  Every list is reached through bitmap words: its own bitmap, or — a list without
// one — bits scattered into the batch's scratch (count_scatter_kernel); tq_docset.hip counts, scans and writes.
// tq_docset_scored_batch*: the same rows with every doc's BM25 score (Weight::for_each, src/query/weight.rs:9-18,89-97):
// tq_docset_score.hip's pass behind every write pass, over a scoring descriptor of its own (score_expression).
// Option "docset_trees": a phrase or a nested boolean query (unscored calls) is planned by plan_tree_query, its exact match
// bits are written into ONE slot of the same scratch by tq_docset_tree.hip behind the sub-batch's scatter, and the
// passes see one Must list that is bits in scratch.  The host variant with one sub-batch keeps the bits between its
// count and write passes, so positions are walked once; with several sub-batches each one is evaluated twice, like the
// scattered lists.
// Option "docset_score_trees": the same shapes in the scored calls.  The tree is planned from the caller's weights, its
// tf_cache joins the batch's cache blob, and tq_docset_tree_score.hip scores its rows behind every sub-batch's write pass,
// next to the flat pass — which is launched over the runs of flat queries between the trees and so writes nothing over a
// tree's row.  The lists' tables (their own or the probe pool's) live for the whole call; only the result bits are the
// sub-batch's, and the scoring pass does not read them.
// A SortSpec (tq_search_sorted_batch*, tq_sort.cpp): everything in front of a sub-batch's passes is the same — checks,
// expressions, tree / slop planning, sub-batches, scatter, tree bits — and the selection launch(es) of tq_sort.hip take the
// place of its count / scan / write passes; the rows go to the spec's device arrays under the caller's query index.
// An AggSpec (tq_agg_batch*, tq_agg.cpp) is taken the same way: the aggregation launch of tq_agg.hip per sub-batch, behind
// one launch that initialises the records and bucket rows of the whole batch.
#include "tq_internal.hpp"

#include <deque>
#include <unordered_map>

namespace tqi {

int docset_expression(tq_segment *s, const tq_query &q, TqkDocsetQuery &dq, const char **why, FlatClauses *fc_out) {
  dq = TqkDocsetQuery{};
  FlatClauses fc_own;
  FlatClauses &fc = fc_out ? *fc_out : fc_own;
  const int prc = parse_flat_clauses(s, q, fc, why);
  if (prc != FLAT_OK) return prc;
  using Clause = FlatClauses::Clause;
  // BooleanWeight::complex_scorer (boolean_weight.rs:236-431), as count_expression restates it
  uint32_t msm = fc.msm;
  if (!fc.all_based && (fc.empty || msm > fc.n_should || (fc.n_must == 0 && fc.n_should == 0))) {
    dq.min_should = 1;  // no lists, one Should clause wanted: the empty set
    return FLAT_OK;
  }
  const bool should_is_must = !fc.all_based && msm >= 2 && msm == fc.n_should;  // all of them: Must clauses
  if (should_is_must) msm = 0;
  // an ALL-BASED query (tq_all.cpp) is the expression with must = all ones: docset_word's start value
  const bool has_must = fc.n_must > 0 || should_is_must || fc.all_based;
  uint32_t n = 0;
  auto put = [&](const Clause &c, uint32_t kind) {
    for (uint32_t i = 0; i < c.n; ++i) {
      const TermHost &th = s->terms[c.terms[i]];
      if (expression_bitmap(s, th)) {
        dq.dense[n] = (const uint2 *)th.dense_blob;
      } else {  // (the handle for now; the pointer once the sub-batch's scratch slot is known)
        dq.dense[n] = (const uint2 *)(uintptr_t)c.terms[i];
        dq.narrow |= 1u << n;
      }
      dq.kinds |= kind << (2u * n);
      if (i + 1 == c.n) {
        if (kind == TQK_COUNT_MUST) dq.clause_end |= 1u << n;
        if (kind == TQK_COUNT_SHOULD) dq.should_end |= 1u << n;
      }
      ++n;
    }
  };
  for (uint32_t c = 0; c < fc.n_cl; ++c)
    if (fc.cl[c].occur == TQ_MUST || (should_is_must && fc.cl[c].occur == TQ_SHOULD && fc.cl[c].n)) put(fc.cl[c], TQK_COUNT_MUST);
  for (uint32_t c = 0; c < fc.n_cl; ++c)
    if (fc.cl[c].occur == TQ_MUST_NOT && fc.cl[c].n) put(fc.cl[c], TQK_COUNT_NOT);
  // with Must clauses and no minimum the Should lists do not change the doc set
  if (!should_is_must && !(has_must && msm == 0))
    for (uint32_t c = 0; c < fc.n_cl; ++c)
      if (fc.cl[c].occur == TQ_SHOULD && fc.cl[c].n) put(fc.cl[c], TQK_COUNT_SHOULD);
  dq.n_terms = n;
  dq.min_should = has_must ? msm : std::max(msm, 1u);  // (msm >= 2 here: fewer than the n_should <= 16 clauses, so <= 15)
  return FLAT_OK;
}

// The scoring lists of a flat query in the order the unpruned scorers add them up (BooleanWeight::complex_scorer,
// boolean_weight.rs:236-431, under for_each, :521-528): the Must clauses — with the Should clauses that
// minimum_number_should_match == n_should >= 2 turned into Must clauses behind them — sorted by cost, stable
// (intersect_scorers, intersection.rs:31); then the Should clauses in query order.  MustNot lists score nothing.
// Every list with the access path tq_docset_score.hip takes: its bitmap, its range directory, or the block search.
void score_expression(tq_segment *s, const tq_query &q, const FlatClauses &fc, TqkScoreQuery &sq) {
  sq = TqkScoreQuery{};
  using Clause = FlatClauses::Clause;
  const uint32_t msm = fc.msm;
  if (!fc.all_based && (fc.empty || msm > fc.n_should || (fc.n_must == 0 && fc.n_should == 0))) return;  // the empty set
  const bool should_is_must = !fc.all_based && msm >= 2 && msm == fc.n_should;
  const Clause *must[TQ_MAX_TERMS];
  uint32_t n_must = 0;
  for (uint32_t c = 0; c < fc.n_cl; ++c)
    if (fc.cl[c].occur == TQ_MUST) must[n_must++] = &fc.cl[c];
  if (should_is_must)
    for (uint32_t c = 0; c < fc.n_cl; ++c)
      if (fc.cl[c].occur == TQ_SHOULD && fc.cl[c].n) must[n_must++] = &fc.cl[c];
  small_stable_sort(must, must + n_must, [](const Clause *a, const Clause *b) { return a->cost < b->cost; });
  uint32_t n = 0;
  auto put = [&](const Clause &c) {
    for (uint32_t i = 0; i < c.n; ++i) {
      const TermHost &th = s->terms[c.terms[i]];
      sq.handle[n] = c.terms[i];
      sq.weight[n] = q.weights[c.pos[i]];
      uint32_t kind = TQK_SCORE_BLOCKS;
      if (th.set_kind == TermHost::kSet) {  // a term set: its bit, its weight as given (ConstScorer)
        kind = TQK_SCORE_CONST;
        sq.tab[n] = th.dense_blob;
      } else if (th.dense_blob && s->opt.use_dense) {
        kind = TQK_SCORE_BITMAP;
        sq.tab[n] = th.dense_blob;
        sq.aux[n] = th.tf8_blob;
      } else if (th.rdir_blob && th.rdir_ent) {
        kind = TQK_SCORE_RDIR;
        sq.tab[n] = th.rdir_blob;
        sq.aux[n] = th.rdir_ent;
        sq.shift[n] = th.rdir_shift;
      }
      sq.shift[n] |= (uint32_t)th.field << 8;  // (multi-field segments: the list's field, read by docset_score_fields_kernel alone)
      sq.access |= kind << (2u * n);
      if (i + 1 == c.n) sq.clause_end |= 1u << n;
      ++n;
    }
  };
  for (uint32_t c = 0; c < n_must; ++c) put(*must[c]);
  sq.n_must_lists = n;
  if (!should_is_must)
    for (uint32_t c = 0; c < fc.n_cl; ++c)
      if (fc.cl[c].occur == TQ_SHOULD && fc.cl[c].n) put(fc.cl[c]);
  sq.n_lists = n;
  // an ALL-BASED query: the sum of the present Should clauses, then + base (a doc that no Should list holds: the base)
  if (fc.all_based) memcpy(&sq.all_base_bits, &fc.all_base, sizeof(float));
}

void docset_tree_view(const tq_query &q, TreeView &v, bool scored) {
  static_assert(TQ_MAX_TERMS == 16, "kOnes holds one weight per term");
  static const float kOnes[TQ_MAX_TERMS] = {1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f};
  v.q = q;
  if (!scored) v.q.weights = kOnes;  // (plan_tree_query reads them and refuses negative boosts: a doc set has neither)
  if (q.mode != TQ_MODE_PHRASE) return;
  if (scored) {  // the phrase's weight on every term: the kernel reads the atom's weight at its first PRESENT term
    for (uint32_t i = 0; i < TQ_MAX_TERMS; ++i) v.weights[i] = q.n_terms ? q.weights[0] : 1.0f;
    v.q.weights = v.weights;
  }
  for (uint32_t i = 0; i < q.n_terms && i < TQ_MAX_TERMS; ++i) {
    v.occurs[i] = TQ_MUST;
    v.clause_of[i] = v.atom_of[i] = 0;
    v.nested_occurs[i] = TQ_MUST | TQ_NESTED_PHRASE;
  }
  v.q.mode = TQ_MODE_BOOL;
  v.q.occurs = v.occurs;
  v.q.clause_of = v.clause_of;
  v.q.atom_of = v.atom_of;
  v.q.nested_occurs = v.nested_occurs;
  v.q.clause_min_should = nullptr;
  v.q.min_should_match = 0;
}

namespace {

struct SubBatch {  // consecutive whole queries whose lists without a bitmap and tree results fit the scratch together
  uint32_t q0 = 0, q1 = 0;
  size_t wg0 = 0, wg1 = 0;  // its part of the scatter work list
  uint32_t t0 = 0, t1 = 0;  // ... and of the tree records (tq_docset_tree.hip)
  uint32_t s0 = 0, s1 = 0;  // ... and of the sloppy phrases' records (tq_phrase_slop.hip)
  bool any_phrase = false;  // some tree of its queries has a phrase atom
  uint32_t n_temp = 0;
  bool score_blocks = false;  // some scoring list of its queries is reached by the block search
};
enum : uint32_t { DS_SCATTER = 1u, DS_COUNT = 2u, DS_WRITE = 4u };

}  // namespace

int docset_batch(tq_segment *s, const tq_query *queries, uint32_t n_queries, uint32_t *out_docs, float *out_scores,
                 uint64_t out_cap, uint64_t *out_starts, bool scored, bool device_out, void *hip_stream, bool count_only,
                 const uint32_t *caller_q, uint32_t n_caller, const SortSpec *sort, const AggSpec *agg) {
  // (tq_count_batch hands over a sub-array of its batch: what this call says about a sloppy phrase — refusals, the
  // overflow words — it says under the CALLER's index)
  auto named = [&](uint32_t qi) { return caller_q ? caller_q[qi] : qi; };
  const uint32_t n_over_words = caller_q ? n_caller : n_queries;
  const char *const fn = sort ? sort->fn : agg ? agg->fn : count_only ? "tq_count_batch" : scored ? (device_out ? "tq_docset_scored_batch_device" : "tq_docset_scored_batch")
                                : (device_out ? "tq_docset_batch_device" : "tq_docset_batch");
  // the write pass stages the docs of a (query, tile) in LDS when the tile holds at least this many (of 65 536)
  static const uint32_t kStageMin = tune_u32("TQ_DOCSET_STAGE_MIN", 2048);
  static const uint64_t kTempBudget = (uint64_t)std::max<uint32_t>(1u, tune_u32("TQ_COUNT_TEMP_MB", 1024)) << 20;
  const uint32_t n_words = (uint32_t)(((uint64_t)s->max_doc + 31u) / 32u);
  const uint32_t words_per_list = (n_words + 63u) & ~63u;
  const uint32_t n_tiles = (n_words + tqk_docset_tile_words() - 1u) / tqk_docset_tile_words();
  uint32_t max_temp = s->opt.docset_temp_lists > 0
                          ? (uint32_t)s->opt.docset_temp_lists
                          : (uint32_t)std::min<uint64_t>(4096u, kTempBudget / std::max<uint64_t>(1u, (uint64_t)words_per_list * 4u));
  max_temp = std::max<uint32_t>(max_temp, TQ_MAX_TERMS);  // a single query always fits
  const uint32_t max_sub_queries = std::max<uint32_t>(1u, (1u << 26) / std::max(1u, n_tiles));  // (query, tile) entries per launch

  // every query is checked before anything is launched: a batch fails as a whole
  std::vector<TqkDocsetQuery> dqs(n_queries);
  std::vector<TqkScoreQuery> sqs(scored ? n_queries : 0u);
  std::vector<const float *> caches;  // the batch's Bm25Weight caches in order of first use (pointer identity, as in search)
  // (a multi-field segment: tf_cache is one row per field, the rows go up together and the index names row 0)
  const uint32_t cache_rows = s->n_fields;
  auto cache_index = [&](const float *tc) {
    for (size_t ci = caches.size(); ci >= cache_rows; ci -= cache_rows)  // (last first: neighbours share one)
      if (caches[ci - cache_rows] == tc) return (uint32_t)(ci - cache_rows);
    for (uint32_t f = 0; f < cache_rows; ++f) caches.push_back(tc + (size_t)f * 256u);
    return (uint32_t)(caches.size() - cache_rows);
  };
  const bool fields = s->n_field_terms != 0;  // (0: no query is looked at for fields)
  bool score_fields = false;                  // some scoring list of the batch belongs to a non-primary field
  uint64_t algo_bytes = 0;
  std::vector<uint32_t> tree_q;     // the queries that take the tree path (option "docset_trees"), ascending
  std::vector<TqdTreeQuery> tqs;    // ... and their records, in the same order
  const bool trees_on = count_only ? false : scored ? s->opt.docset_score_trees != 0 : s->opt.docset_trees != 0;
  // Sloppy phrases (TQ_MODE_PHRASE with slop > 0, tq_phrase_slop.cpp): the existence verdict of the reference's non-scoring
  // PhraseScorer as match bits in a result slot of their own, like a tree's: phrase_slop_bits_kernel stores every word of
  // it, once (a query the planner found empty: zeros).  Taken by
  // the unscored calls under "docset_trees" and by the count pass of tq_count_batch.
  std::deque<SlopView> slop_views;
  std::vector<uint32_t> slop_qi;         // the sloppy phrases of the batch, ascending
  std::vector<TqdSlopQuery> slop_qs;     // ... and their records, in the same order
  s->last_batch_slop = false;
  s->slop_over_words = n_over_words;
  for (uint32_t qi = 0; qi < n_queries; ++qi) {
    const char *why = "";
    FlatClauses fc;
    const tq_query &q = queries[qi];
    if (q.slop) {
      slop_views.emplace_back();
      const int vrc = slop_view(s, q, named(qi), fn, slop_views.back(), false);
      if (vrc != TQ_OK) return vrc;
      if (scored)
        return fail(TQ_ERR_UNSUPPORTED, "%s: query %u: scored doc sets of sloppy phrases stay on the CPU in this version", fn, named(qi));
      if (!trees_on && !count_only)
        return fail(TQ_ERR_UNSUPPORTED, "%s: query %u is a phrase: doc sets of phrases and nested queries stay on the CPU (option \"docset_trees\")", fn, named(qi));
      slop_qi.push_back(qi);
      continue;
    }
    {  // a term set in a phrase, inside a nested query, or released: refused whatever the tree options say
      bool names_set = false;
      const int src = check_set_query(s, q, qi, fn, &names_set);
      if (src != TQ_OK) return src;
    }
    const bool names_field = fields && query_names_field(s, q);
    if (names_field) {  // a phrase over two fields: refused whatever the tree options say
      const int frc = check_field_query(s, q, qi, fn);
      if (frc != TQ_OK) return frc;
    }
    const int rc = docset_expression(s, q, dqs[qi], &why, scored ? &fc : nullptr);
    if (rc == FLAT_UNSUPPORTED && trees_on && !query_has_all(q) && (q.mode == TQ_MODE_PHRASE || bool_query_is_tree(q))) {
      if (scored && names_field)  // (docset_tree_score_kernel scores under the primary field's norms)
        return fail(TQ_ERR_UNSUPPORTED, "%s: query %u: scored doc sets of phrases and nested queries that name a non-primary field stay on the CPU in this version", fn, qi);
      if (scored) {  // the rule of the flat queries; plan_tree_query reads every term's weight
        if (!q.weights || !q.tf_cache) return fail(TQ_ERR_INVALID, "%s: query %u: null weights / tf_cache", fn, qi);
        for (uint32_t i = 0; i < (q.mode == TQ_MODE_PHRASE ? std::min(q.n_terms, 1u) : q.n_terms); ++i)
          if (!std::isfinite(q.weights[i])) return fail(TQ_ERR_INVALID, "%s: query %u: weight %u is not finite", fn, qi, i);
      }
      tree_q.push_back(qi);
      continue;
    }
    if (rc == FLAT_UNSUPPORTED)
      return fail(TQ_ERR_UNSUPPORTED, "%s: query %u is %s: doc sets of phrases and nested queries stay on the CPU", fn, qi, why);
    if (rc != FLAT_OK) return fail(TQ_ERR_INVALID, "%s: query %u: %s", fn, qi, why);
    algo_bytes += (uint64_t)dqs[qi].n_terms * n_words * 4u;
    if (!scored) continue;
    bool has_list = false;
    for (uint32_t c = 0; c < fc.n_cl; ++c) has_list = has_list || (fc.cl[c].occur != TQ_MUST_NOT && fc.cl[c].n);
    if (has_list && (!q.weights || !q.tf_cache)) return fail(TQ_ERR_INVALID, "%s: query %u: null weights / tf_cache", fn, qi);
    if (has_list)
      for (uint32_t i = 0; i < q.n_terms; ++i)
        if (!std::isfinite(q.weights[i])) return fail(TQ_ERR_INVALID, "%s: query %u: weight %u is not finite", fn, qi, i);
    if (fc.all_boost_mixed)
      return fail(TQ_ERR_UNSUPPORTED, "%s: query %u has a boosted match-all clause beside another scoring clause or a second match-all clause: its scores stay on the CPU",
                  fn, qi);
    if (has_list || fc.all_based) score_expression(s, q, fc, sqs[qi]);
    if (sqs[qi].n_lists) sqs[qi].cache_idx = cache_index(q.tf_cache);
    for (uint32_t m = 0; names_field && m < sqs[qi].n_lists; ++m) score_fields = score_fields || (sqs[qi].shift[m] >> 8) != 0u;
    algo_bytes += (uint64_t)sqs[qi].n_lists * n_words * 8u;
  }
  if (!tree_q.empty() || !slop_qi.empty()) {
    // every list of a tree as a bitmap + tf bytes, a phrase term's position directory: the list's own tables or the probe
    // pool's, built now; a probe batch like a search batch's, so that no list of this call is evicted for another
    probe_begin_batch(s);
    std::deque<TreeView> views;
    bool built = false;
    for (const uint32_t qi : tree_q) {
      views.emplace_back();
      docset_tree_view(queries[qi], views.back(), scored);
      const int prc = build_tree_query_probe_tables(s, views.back().q, &built);
      if (prc != TQ_OK) return prc;
    }
    for (const SlopView &sv : slop_views) {
      const int prc = build_tree_query_probe_tables(s, sv.v.q, &built);
      if (prc != TQ_OK) return prc;
    }
    if (built) s->share_span_terms = ~(size_t)0;
    update_table_span(s);
    if (!s->share_span_ok || !s->opt.use_dense)
      return fail_tree_tables(s, named(std::min(tree_q.empty() ? ~0u : tree_q[0], slop_qi.empty() ? ~0u : slop_qi[0])));
    tqs.resize(tree_q.size());
    slop_qs.resize(slop_qi.size());
    for (size_t k = 0; k < slop_qi.size(); ++k) {
      // (named: the query in refusals, and its overflow word; the lists' bits once + the result word written and read back)
      const int prc = plan_slop_query(s, slop_views[k].v.q, named(slop_qi[k]), queries[slop_qi[k]].slop, slop_qs[k], algo_bytes, true);
      if (prc != TQ_OK) return prc;
      TqkDocsetQuery &dq = dqs[slop_qi[k]];  // to the passes: one Must list that is bits in scratch
      dq = TqkDocsetQuery{};
      dq.n_terms = dq.narrow = dq.clause_end = 1u;
    }
    for (size_t i = 0; i < tree_q.size(); ++i) {
      uint64_t qbytes = 0;
      const int prc = plan_tree_query(s, views[i].q, tree_q[i], tqs[i], qbytes, s->share_table_lo);
      if (prc != TQ_OK) return prc;  // (names the query)
      TqkDocsetQuery &dq = dqs[tree_q[i]];  // to the passes: one Must list that is bits in scratch
      dq = TqkDocsetQuery{};
      dq.n_terms = dq.narrow = dq.clause_end = 1u;
      // every list's bits once + the result word written and read back
      algo_bytes += ((uint64_t)tqs[i].n_terms + 2u) * n_words * 4u;
      if (!scored) continue;
      if (tqs[i].n_terms) {  // its cache in the blob the flat queries use: one index space for both scoring kernels
        tqs[i].cache_idx = cache_index(queries[tree_q[i]].tf_cache);
      }
      // the scoring pass: one bitmap word per 32 docs for every list that scores (under no MustNot on either level)
      uint32_t n_scoring = 0;
      for (uint32_t c = 0; c < tqs[i].n_clauses; ++c)
        for (uint32_t t = tqs[i].first_term[c]; t < tqs[i].first_term[c + 1u]; ++t)
          n_scoring += tqs[i].outer[c] != TQ_MUST_NOT && tqs[i].inner[t] != TQ_MUST_NOT ? 1u : 0u;
      algo_bytes += (uint64_t)n_scoring * n_words * 8u;
    }
  }
  // sub-batches; a list without a bitmap gets a slot of the scratch for the duration of its sub-batch
  std::vector<SubBatch> subs;
  std::vector<uint4> wgs;
  std::unordered_map<uint32_t, uint32_t> slot;
  SubBatch cur;
  uint32_t max_sub_temp = 0, max_sub_n = 0;
  uint32_t n_slots = 0;  // slots of the sub-batch so far: its lists without a bitmap and its trees' results
  uint32_t n_trees = 0;  // tree queries so far
  uint32_t n_slops = 0;  // sloppy phrases so far
  auto close_sub = [&](uint32_t q1) {
    cur.q1 = q1;
    cur.wg1 = wgs.size();
    cur.t1 = n_trees;
    cur.s1 = n_slops;
    cur.n_temp = n_slots;
    for (uint32_t qi = cur.q0; scored && qi < q1; ++qi)
      for (uint32_t m = 0; m < sqs[qi].n_lists; ++m)
        cur.score_blocks = cur.score_blocks || ((sqs[qi].access >> (2u * m)) & 3u) == TQK_SCORE_BLOCKS;
    max_sub_temp = std::max(max_sub_temp, cur.n_temp);
    max_sub_n = std::max(max_sub_n, cur.q1 - cur.q0);
    subs.push_back(cur);
    cur = SubBatch{};
    cur.q0 = q1;
    cur.wg0 = wgs.size();
    cur.t0 = n_trees;
    cur.s0 = n_slops;
    slot.clear();
    n_slots = 0;
  };
  for (uint32_t qi = 0; qi < n_queries; ++qi) {
    TqkDocsetQuery &dq = dqs[qi];
    if (n_trees < tree_q.size() && tree_q[n_trees] == qi) {  // a tree: one result slot, like a fresh list
      if (qi > cur.q0 && (n_slots + 1u > max_temp || qi - cur.q0 >= max_sub_queries)) close_sub(qi);
      cur.any_phrase = cur.any_phrase || tqs[n_trees].has_phrase;
      tqs[n_trees++].part_start = n_slots;
      dq.dense[0] = (const uint2 *)(uintptr_t)n_slots++;  // (the slot; the pointer below)
      continue;
    }
    if (n_slops < slop_qi.size() && slop_qi[n_slops] == qi) {  // a sloppy phrase: one result slot too
      if (qi > cur.q0 && (n_slots + 1u > max_temp || qi - cur.q0 >= max_sub_queries)) close_sub(qi);
      slop_qs[n_slops++].part_start = n_slots;
      dq.dense[0] = (const uint2 *)(uintptr_t)n_slots++;
      continue;
    }
    uint32_t fresh[TQ_MAX_TERMS], n_fresh = 0;
    for (uint32_t m = 0; m < dq.n_terms; ++m) {
      if (!((dq.narrow >> m) & 1u)) continue;
      const uint32_t h = (uint32_t)(uintptr_t)dq.dense[m];
      if (slot.count(h) || std::find(fresh, fresh + n_fresh, h) != fresh + n_fresh) continue;
      fresh[n_fresh++] = h;
    }
    if (qi > cur.q0 && (n_slots + n_fresh > max_temp || qi - cur.q0 >= max_sub_queries)) close_sub(qi);
    for (uint32_t m = 0; m < dq.n_terms; ++m) {
      if (!((dq.narrow >> m) & 1u)) continue;
      const uint32_t h = (uint32_t)(uintptr_t)dq.dense[m];
      auto it = slot.find(h);
      if (it == slot.end()) {
        it = slot.emplace(h, n_slots++).first;
        for (uint32_t j = 0; j < s->terms[h].n_blocks; j += 4u) wgs.push_back(make_uint4(h, j, it->second, 0u));
      }
      dq.dense[m] = (const uint2 *)(uintptr_t)it->second;  // (the slot; the pointer below)
    }
  }
  if (n_queries) close_sub(n_queries);

  HIP_TRY(hipSetDevice(s->device));
  hipStream_t st = device_out && hip_stream ? (hipStream_t)hip_stream : s->stream;
  {
    const int wrc = wait_segment_idle(s);  // the scratch below is shared with the batches before
    if (wrc != TQ_OK) return wrc;
  }
  s->stats = tq_batch_stats{};
  s->stats.kernel_mask = (sort ? TQ_KERNEL_SORT : agg ? TQ_KERNEL_AGG : TQ_KERNEL_DOCSET) | (scored ? TQ_KERNEL_DOCSET_SCORE : 0u) | (tqs.empty() ? 0u : TQ_KERNEL_DOCSET_TREE) |
                         (scored && !tqs.empty() ? TQ_KERNEL_DOCSET_TREE_SCORE : 0u) | (slop_qs.empty() ? 0u : TQ_KERNEL_PHRASE_SLOP);
  s->stats.algorithmic_bytes = algo_bytes;
  if (agg) s->stats.algorithmic_bytes += (uint64_t)n_queries * (sizeof(tq_agg_stats_t) + 4u * (uint64_t)agg->plan.n_buckets);
  s->stats_pending = false;
  s->last_batch_queries = 0;
  if (!sort && !agg && (n_queries == 0 || n_tiles == 0)) {  // no query, or a segment without docs: empty rows
    if (device_out) {
      HIP_TRY(hipMemsetAsync(out_starts, 0, ((size_t)n_queries + 1u) * sizeof(uint64_t), st));
    } else {
      memset(out_starts, 0, ((size_t)n_queries + 1u) * sizeof(uint64_t));
    }
    return TQ_OK;
  }
  if (!wgs.empty() || scored || !tqs.empty() || !slop_qs.empty()) {  // (the scoring pass reads term records: saturated tfs, the block search; a phrase atom: positions)
    const int src = sync_terms(s, s->stream);
    if (src != TQ_OK) return src;
  }
  const size_t q_bytes = (size_t)n_queries * sizeof(TqkDocsetQuery), wg_bytes = wgs.size() * sizeof(uint4);
  const size_t sq_bytes = sqs.size() * sizeof(TqkScoreQuery), cache_bytes = caches.size() * 256u * sizeof(float);
  const size_t tree_bytes = tqs.size() * sizeof(TqdTreeQuery);
  // scored: behind the records, which query of its sub-batch every tree is (tq_docset_tree_score.hip: tile_counts / tile_offs)
  static_assert(sizeof(TqdTreeQuery) % sizeof(uint32_t) == 0, "the map stands right behind the records");
  const size_t tree_map_bytes = scored ? tqs.size() * sizeof(uint32_t) : 0u;
  const size_t max_entries = (size_t)max_sub_n * n_tiles;
  // (the sloppy phrases' records ride behind the tree records and their map, 64-byte aligned, in both buffers)
  const size_t slop_off = (tree_bytes + tree_map_bytes + 63u) & ~(size_t)63, slop_bytes = slop_qs.size() * sizeof(TqdSlopQuery);
  const size_t tree_blob_bytes = slop_bytes ? slop_off + slop_bytes : tree_bytes + tree_map_bytes;
  // the slices per query of a sorted or an aggregation call: enough workgroups for the machine, no slice below four steps
  // of the walk (1024 words), or what "sort_slices" / "agg_slices" forces
  auto pick_slices = [&](int forced, uint32_t step_words) -> uint32_t {
    if (forced > 0) return (uint32_t)forced;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, s->device) != hipSuccess || cus <= 0) cus = 256;
    const uint32_t want = ((uint32_t)cus * 4u + max_sub_n - 1u) / std::max(1u, max_sub_n);
    return std::max(1u, std::min({want, 256u, n_words / (4u * step_words)}));
  };
  // a sorted call: its slices, the key slots per lane its largest k needs, and every query's k behind the blobs above
  uint32_t sort_slices = 1, sort_wps = n_words, sort_kpl = 1;
  const size_t ks_off = ((q_bytes + wg_bytes + sq_bytes + cache_bytes + 63u) & ~(size_t)63) + ((tree_blob_bytes + 63u) & ~(size_t)63);
  const size_t ks_bytes = sort ? (size_t)n_queries * sizeof(uint32_t) : 0u;
  if (sort) {
    uint32_t max_k = 1;
    for (uint32_t qi = 0; qi < n_queries; ++qi) max_k = std::max(max_k, queries[qi].k);
    sort_kpl = max_k <= 64u ? 1 : max_k <= 256u ? 4 : 16;
    sort_slices = pick_slices(s->opt.sort_slices, tqk_sort_step_words());
    sort_wps = (n_words + sort_slices - 1u) / sort_slices;
  }
  // an aggregation call: its slices
  uint32_t agg_slices = 1, agg_wps = n_words;
  if (agg) {
    agg_slices = pick_slices(s->opt.agg_slices, tqk_agg_step_words());
    agg_wps = (n_words + agg_slices - 1u) / agg_slices;
  }
  const size_t sort_part_bytes = sort_slices > 1u ? (size_t)max_sub_n * sort_slices * (size_t)sort_kpl * 64u * 2u * sizeof(uint64_t) : 0u;
  int rc = s->h_docset.ensure(ks_off + ks_bytes + 64u);
  if (rc == TQ_OK && sort) rc = s->d_sort_ks.ensure(ks_bytes);
  if (rc == TQ_OK && sort_part_bytes) rc = s->d_sort_partials.ensure(sort_part_bytes);
  if (rc == TQ_OK && sort_part_bytes) rc = s->d_sort_slice_counts.ensure((size_t)max_sub_n * sort_slices * sizeof(uint2));
  if (rc == TQ_OK && tree_blob_bytes) rc = s->d_docset_trees.ensure(tree_blob_bytes);
  if (rc == TQ_OK && slop_bytes) rc = s->d_slop_over.ensure((size_t)n_over_words * sizeof(uint32_t));
  if (rc == TQ_OK && scored) rc = s->d_docset_squeries.ensure(sq_bytes);
  if (rc == TQ_OK && scored) rc = s->d_docset_caches.ensure(std::max<size_t>(cache_bytes, 256u * sizeof(float)));
  if (rc == TQ_OK) rc = s->d_docset_queries.ensure(q_bytes);
  if (rc == TQ_OK) rc = s->d_count_wgs.ensure(wg_bytes);
  if (rc == TQ_OK) rc = s->d_count_bits.ensure((size_t)max_sub_temp * words_per_list * sizeof(uint32_t));
  if (rc == TQ_OK && !sort && !agg) rc = s->d_docset_counts.ensure(max_entries * sizeof(uint32_t));
  if (rc == TQ_OK && !sort && !agg) rc = s->d_docset_offs.ensure(max_entries * sizeof(uint64_t));
  if (rc == TQ_OK && !sort && !agg) rc = s->d_docset_partials.ensure(((max_entries + tqk_docset_scan_tile() - 1) / tqk_docset_scan_tile()) * sizeof(uint64_t));
  if (rc == TQ_OK) rc = s->d_qmatches.ensure((size_t)n_queries * sizeof(uint32_t));
  if (rc == TQ_OK && !device_out) rc = s->d_docset_starts.ensure(((size_t)n_queries + 1u) * sizeof(uint64_t));
  if (rc != TQ_OK) return rc;
  for (TqkDocsetQuery &dq : dqs)
    for (uint32_t m = 0; m < dq.n_terms; ++m)
      if ((dq.narrow >> m) & 1u)
        dq.dense[m] = (const uint2 *)((const uint32_t *)s->d_count_bits.p + (size_t)(uintptr_t)dq.dense[m] * words_per_list);
  // option "timing" (device variant): the batch takes a slot of the event ring like a search batch
  const bool timed = device_out && s->opt.timing;
  const int ring = (int)(s->batches_timed % tq_segment::kTimingRing);
  if (timed) HIP_TRY(hipEventRecord(s->ev_t0[ring], st));
  memcpy(s->h_docset.p, dqs.data(), q_bytes);
  if (wg_bytes) memcpy((uint8_t *)s->h_docset.p + q_bytes, wgs.data(), wg_bytes);
  HIP_TRY(hipMemcpyAsync(s->d_docset_queries.p, s->h_docset.p, q_bytes, hipMemcpyHostToDevice, st));
  if (wg_bytes)
    HIP_TRY(hipMemcpyAsync(s->d_count_wgs.p, (const uint8_t *)s->h_docset.p + q_bytes, wg_bytes, hipMemcpyHostToDevice, st));
  if (scored) {
    uint8_t *const h_sq = (uint8_t *)s->h_docset.p + q_bytes + wg_bytes;
    memcpy(h_sq, sqs.data(), sq_bytes);
    for (size_t c = 0; c < caches.size(); ++c) memcpy(h_sq + sq_bytes + c * 256u * sizeof(float), caches[c], 256u * sizeof(float));
    HIP_TRY(hipMemcpyAsync(s->d_docset_squeries.p, h_sq, sq_bytes, hipMemcpyHostToDevice, st));
    if (cache_bytes) HIP_TRY(hipMemcpyAsync(s->d_docset_caches.p, h_sq + sq_bytes, cache_bytes, hipMemcpyHostToDevice, st));
  }
  if (tree_blob_bytes) {
    uint8_t *const h_tq = (uint8_t *)s->h_docset.p + q_bytes + wg_bytes + sq_bytes + cache_bytes;
    if (tree_bytes) memcpy(h_tq, tqs.data(), tree_bytes);
    if (tree_map_bytes) {
      uint32_t *const map = (uint32_t *)(h_tq + tree_bytes);
      for (const SubBatch &sb : subs)
        for (uint32_t t = sb.t0; t < sb.t1; ++t) map[t] = tree_q[t] - sb.q0;
    }
    if (slop_bytes) memcpy(h_tq + slop_off, slop_qs.data(), slop_bytes);
    HIP_TRY(hipMemcpyAsync(s->d_docset_trees.p, h_tq, tree_blob_bytes, hipMemcpyHostToDevice, st));
  }
  if (sort) {  // every query's k, and the three totals the selection adds to
    uint32_t *const h_ks = (uint32_t *)((uint8_t *)s->h_docset.p + ks_off);
    for (uint32_t qi = 0; qi < n_queries; ++qi) h_ks[qi] = queries[qi].k;
    HIP_TRY(hipMemcpyAsync(s->d_sort_ks.p, h_ks, ks_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(s->d_match_counter, 0, 3u * sizeof(unsigned long long), st));
  }
  if (agg) {  // what the aggregation launches add to: the totals, every query's match count, the records and bucket rows
    HIP_TRY(hipMemsetAsync(s->d_match_counter, 0, 3u * sizeof(unsigned long long), st));
    HIP_TRY(hipMemsetAsync(s->d_qmatches.p, 0, (size_t)n_queries * sizeof(uint32_t), st));
    const hipError_t ie = tqk_launch_agg_init((TqkAggStats *)agg->d_stats, agg->d_buckets, n_queries, agg->plan.n_buckets,
                                              agg->bucket_stride, st);
    if (ie != hipSuccess) return fail(TQ_ERR_HIP, "aggregation init launch: %s", hipGetErrorString(ie));
  }
  if (slop_bytes) {  // the overflow words, one per query of the batch (tq_last_batch_slop_overflows)
    HIP_TRY(hipMemsetAsync(s->d_slop_over.p, 0, (size_t)n_over_words * sizeof(uint32_t), st));
    s->last_batch_slop = true;
  }

  uint64_t *const d_starts = device_out ? out_starts : (uint64_t *)s->d_docset_starts.p;
  auto enqueue = [&](const SubBatch &sb, uint32_t stages, uint32_t *d_docs, float *d_scores, uint64_t cap) -> int {
    if ((stages & DS_SCATTER) && sb.wg1 > sb.wg0) {  // the sub-batch's lists without a bitmap, as bits
      HIP_TRY(hipMemsetAsync(s->d_count_bits.p, 0, (size_t)sb.n_temp * words_per_list * sizeof(uint32_t), st));
      const hipError_t se = tqk_launch_count_scatter(s->dseg, s->d_terms, (const uint4 *)s->d_count_wgs.p + sb.wg0,
                                                     (uint32_t)(sb.wg1 - sb.wg0), (uint32_t *)s->d_count_bits.p, words_per_list, st);
      if (se != hipSuccess) return fail(TQ_ERR_HIP, "doc-set scatter launch: %s", hipGetErrorString(se));
    }
    if ((stages & DS_SCATTER) && sb.t1 > sb.t0) {  // its trees' match bits: every word of their slots is stored, once
      TqkDocsetTreeParams tp{};
      tp.seg = s->dseg;
      tp.terms = s->d_terms;
      tp.queries = (const TqdTreeQuery *)s->d_docset_trees.p + sb.t0;
      tp.table_base = (const uint8_t *)s->share_table_lo;
      tp.bits = (uint32_t *)s->d_count_bits.p;
      tp.n_queries = sb.t1 - sb.t0;
      tp.n_words = n_words;
      tp.words_per_list = words_per_list;
      tp.any_phrase = sb.any_phrase ? 1u : 0u;
      const hipError_t te = tqk_launch_docset_tree(tp, st);
      if (te != hipSuccess) return fail(TQ_ERR_HIP, "doc-set tree launch: %s", hipGetErrorString(te));
    }
    if ((stages & DS_SCATTER) && sb.s1 > sb.s0) {  // its sloppy phrases' match bits: every word of their slots is stored, once
      TqkPhraseSlopParams pp{};
      pp.seg = s->dseg;
      pp.terms = s->d_terms;
      pp.queries = (const TqdSlopQuery *)((const uint8_t *)s->d_docset_trees.p + slop_off) + sb.s0;
      pp.table_base = (const uint8_t *)s->share_table_lo;
      pp.overflow = (uint32_t *)s->d_slop_over.p;
      pp.bits = (uint32_t *)s->d_count_bits.p;
      pp.n_queries = sb.s1 - sb.s0;
      pp.n_words = n_words;
      pp.words_per_list = words_per_list;
      for (uint32_t k = sb.s0; k < sb.s1; ++k) (slop_qs[k].n_terms > 2u ? pp.any_carry : pp.any_pair) = 1u;
      const hipError_t pe = tqk_launch_phrase_slop_bits(pp, st);
      if (pe != hipSuccess) return fail(TQ_ERR_HIP, "sloppy phrase launch: %s", hipGetErrorString(pe));
    }
    TqkDocsetParams p{};
    p.queries = (const TqkDocsetQuery *)s->d_docset_queries.p + sb.q0;
    p.alive = s->d_alive;
    p.tile_counts = (uint32_t *)s->d_docset_counts.p;
    p.tile_offs = (uint64_t *)s->d_docset_offs.p;
    p.partials = (uint64_t *)s->d_docset_partials.p;
    p.base_in = sb.q0 ? d_starts + sb.q0 : nullptr;  // (the total the sub-batch before left there)
    p.out_starts = d_starts + sb.q0;
    p.query_sizes = (uint32_t *)s->d_qmatches.p + sb.q0;
    p.total_out = s->d_match_counter;
    p.out_docs = d_docs;
    p.out_cap = cap;
    p.n_queries = sb.q1 - sb.q0;
    p.n_tiles = n_tiles;
    p.n_words = n_words;
    p.max_doc = s->max_doc;
    p.stage_min_docs = kStageMin;
    hipError_t e = hipSuccess;
    if (sort) {  // the selection in place of the count / scan / write passes: rows under the caller's query index
      const tq_segment::ColumnHost &col = s->columns[sort->column];
      TqkSortParams sp{};
      sp.ds = p;
      sp.col = col.dev;
      sp.min_value = col.info.min_value;
      sp.gcd = col.info.gcd;
      sp.ks = (const uint32_t *)s->d_sort_ks.p + sb.q0;
      sp.partials = (uint64_t *)s->d_sort_partials.p;
      sp.slice_counts = (uint2 *)s->d_sort_slice_counts.p;
      sp.out_docs = sort->d_docs + (size_t)sb.q0 * sort->out_stride;
      sp.out_values = sort->d_values + (size_t)sb.q0 * sort->out_stride;
      sp.out_has_value = sort->d_has_value + (size_t)sb.q0 * sort->out_stride;
      sp.out_counts = sort->d_counts + sb.q0;
      sp.query_sizes = p.query_sizes;
      sp.totals = s->d_match_counter;
      sp.n_slices = sort_slices;
      sp.words_per_slice = sort_wps;
      sp.out_stride = sort->out_stride;
      sp.ascending = sort->ascending;
      sp.nulls_first = sort->nulls_first;
      e = tqk_launch_sort_select(sp, (int)sort_kpl, st);
      if (e == hipSuccess) e = tqk_launch_sort_merge(sp, (int)sort_kpl, st);
      if (e != hipSuccess) return fail(TQ_ERR_HIP, "sort kernel launch: %s", hipGetErrorString(e));
      return TQ_OK;
    }
    if (agg) {  // the aggregation in place of the count / scan / write passes: records and rows under the caller's query index
      const tq_segment::ColumnHost &col = s->columns[agg->column];
      TqkAggParams ap{};
      ap.ds = p;
      ap.col = col.dev;
      ap.min_value = col.info.min_value;
      ap.gcd = col.info.gcd;
      ap.stats = (TqkAggStats *)agg->d_stats + sb.q0;
      ap.buckets = agg->d_buckets ? agg->d_buckets + (size_t)sb.q0 * agg->bucket_stride : nullptr;
      ap.query_sizes = p.query_sizes;
      ap.totals = s->d_match_counter;
      ap.interval = agg->interval;
      ap.offset = agg->offset;
      ap.bounds_min = agg->plan.bounds_min;
      ap.bounds_max = agg->plan.bounds_max;
      ap.base_pos = agg->plan.base_pos;
      ap.n_buckets = agg->plan.n_buckets;
      ap.bucket_stride = agg->bucket_stride;
      ap.lds_buckets = s->opt.agg_lds_buckets < 0 ? tqk_agg_lds_buckets() : (uint32_t)s->opt.agg_lds_buckets;
      ap.value_type = agg->value_type;
      ap.n_slices = agg_slices;
      ap.words_per_slice = agg_wps;
      e = tqk_launch_agg(ap, st);
      if (e != hipSuccess) return fail(TQ_ERR_HIP, "aggregation kernel launch: %s", hipGetErrorString(e));
      return TQ_OK;
    }
    if (stages & DS_COUNT) {
      e = tqk_launch_docset_count(p, st);
      if (e == hipSuccess) e = tqk_launch_docset_scan(p, st);
    }
    if (e == hipSuccess && (stages & DS_WRITE)) e = tqk_launch_docset_write(p, st);
    if (e == hipSuccess && (stages & DS_WRITE) && scored) {  // right behind its write pass: the tables are this sub-batch's
      TqkScoreParams sp{};
      sp.seg = s->dseg;
      sp.terms = s->d_terms;
      sp.caches = (const float *)s->d_docset_caches.p;
      sp.out_docs = d_docs;
      sp.out_scores = d_scores;
      sp.out_cap = cap;
      sp.n_tiles = n_tiles;
      sp.any_blocks = sb.score_blocks ? 1u : 0u;
      // the flat pass over the runs of flat queries between the sub-batch's trees (no tree: the one launch it always was):
      // a tree's row is the tree pass's alone — the flat kernel would store the empty sum over it
      uint32_t r0 = sb.q0;
      for (uint32_t t = sb.t0; t <= sb.t1 && e == hipSuccess; ++t) {
        const uint32_t r1 = t < sb.t1 ? tree_q[t] : sb.q1;
        if (r1 > r0) {
          sp.queries = (const TqkScoreQuery *)s->d_docset_squeries.p + r0;
          sp.tile_counts = p.tile_counts + (size_t)(r0 - sb.q0) * n_tiles;
          sp.tile_offs = p.tile_offs + (size_t)(r0 - sb.q0) * n_tiles;
          sp.n_queries = r1 - r0;
          if (score_fields) {  // per-list norms (tq_fields.cpp)
            TqkScoreFieldsParams fp{};
            fp.base = sp;
            fp.fn[0] = s->d_fn;
            for (uint32_t f = 1; f < TQK_MAX_FIELDS; ++f) fp.fn[f] = s->d_fn_field[f];
            e = tqk_launch_docset_score_fields(fp, st);
          } else {
            e = tqk_launch_docset_score(sp, st);
          }
        }
        r0 = r1 + 1u;
      }
      if (e == hipSuccess && sb.t1 > sb.t0) {
        TqkDocsetTreeScoreParams tsp{};
        tsp.seg = s->dseg;
        tsp.terms = s->d_terms;
        tsp.queries = (const TqdTreeQuery *)s->d_docset_trees.p + sb.t0;
        tsp.query_of = (const uint32_t *)((const uint8_t *)s->d_docset_trees.p + tree_bytes) + sb.t0;
        tsp.caches = (const float *)s->d_docset_caches.p;
        tsp.table_base = (const uint8_t *)s->share_table_lo;
        tsp.tile_counts = p.tile_counts;
        tsp.tile_offs = p.tile_offs;
        tsp.out_docs = d_docs;
        tsp.out_scores = d_scores;
        tsp.out_cap = cap;
        tsp.n_queries = sb.t1 - sb.t0;
        tsp.n_tiles = n_tiles;
        tsp.any_phrase = sb.any_phrase ? 1u : 0u;
        e = tqk_launch_docset_tree_score(tsp, st);
      }
    }
    if (e != hipSuccess) return fail(TQ_ERR_HIP, "doc-set kernel launch: %s", hipGetErrorString(e));
    return TQ_OK;
  };

  s->last_batch_queries = n_queries;
  if (device_out) {
    if (timed) HIP_TRY(hipEventRecord(s->ev_k0[ring], st));
    for (const SubBatch &sb : subs) {
      rc = enqueue(sb, DS_SCATTER | DS_COUNT | DS_WRITE, out_docs, out_scores, out_cap);
      if (rc != TQ_OK) return rc;
    }
    if (timed) {
      HIP_TRY(hipEventRecord(s->ev_k1[ring], st));
      HIP_TRY(hipEventRecord(s->ev_t1[ring], st));
      ++s->batches_timed;
    }
    s->stats_pending = true;  // the total is on the device: tq_last_batch_stats reads it
    s->stats_match_bytes = scored ? 9 : 4;  // doc [+ score + fieldnorm byte]
    s->stats_sorted = sort || agg;    // (its own byte model: tq_last_batch_stats)
    s->stats_sorted_optional = (sort && s->columns[sort->column].dev.present != nullptr) ||
                               (agg && s->columns[agg->column].dev.present != nullptr);
    HIP_TRY(hipEventRecord(s->ev_batch_done, st));
    s->last_stream = st;
    s->batch_in_flight = true;
    return TQ_OK;
  }
  // host outputs: the row starts first — they say whether the docs fit
  for (const SubBatch &sb : subs) {
    rc = enqueue(sb, DS_SCATTER | DS_COUNT, nullptr, nullptr, 0);
    if (rc != TQ_OK) return rc;
  }
  HIP_TRY(hipMemcpyAsync(out_starts, d_starts, ((size_t)n_queries + 1u) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const uint64_t total = out_starts[n_queries];
  s->stats.matches = total;
  // host outputs wait for the device anyway: a sloppy phrase whose carried list went over the cap is reported, the rows
  // of the other queries are written and valid
  auto slop_verdict = [&]() -> int {
    if (slop_qs.empty()) return TQ_OK;
    std::vector<uint32_t> over(n_over_words);
    HIP_TRY(hipMemcpy(over.data(), s->d_slop_over.p, (size_t)n_over_words * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return slop_overflow_verdict(fn, over.data(), n_over_words);
  };
  if (count_only) return slop_verdict();  // (tq_count_batch: the row starts are the counts)
  s->stats.algorithmic_bytes += (scored ? 9u : 4u) * total;
  if (total > out_cap)
    return fail(TQ_ERR_INVALID, "%s: the batch has %llu docs, out_cap is %llu (out_starts is filled: retry with that many)", fn,
                (unsigned long long)total, (unsigned long long)out_cap);
  if (!total) return slop_verdict();
  rc = s->d_docset_docs.ensure((size_t)total * sizeof(uint32_t));
  if (rc == TQ_OK && scored) rc = s->d_docset_scores.ensure((size_t)total * sizeof(float));
  if (rc != TQ_OK) return rc;
  if (subs.size() > 1 && !slop_qs.empty())  // (evaluated again: the overflow words count every candidate once)
    HIP_TRY(hipMemsetAsync(s->d_slop_over.p, 0, (size_t)n_over_words * sizeof(uint32_t), st));
  for (const SubBatch &sb : subs) {
    // one sub-batch: its tables and bits are still there; several: each is evaluated again (the scratch held the last one's)
    rc = enqueue(sb, subs.size() == 1 ? DS_WRITE : (DS_SCATTER | DS_COUNT | DS_WRITE), (uint32_t *)s->d_docset_docs.p,
                 (float *)s->d_docset_scores.p, total);
    if (rc != TQ_OK) return rc;
  }
  HIP_TRY(hipMemcpyAsync(out_docs, s->d_docset_docs.p, (size_t)total * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  if (scored) HIP_TRY(hipMemcpyAsync(out_scores, s->d_docset_scores.p, (size_t)total * sizeof(float), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (s->d_docset_docs.cap > ((size_t)256 << 20)) s->d_docset_docs.release();  // (a large result is not kept as scratch)
  if (s->d_docset_scores.cap > ((size_t)256 << 20)) s->d_docset_scores.release();
  return slop_verdict();
}

}  // namespace tqi
