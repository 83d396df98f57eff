// tq_docset_batch / tq_docset_batch_device: the full doc set of every query of a batch (Weight::for_each_no_score ->
// SegmentCollector::collect_block with the alive filter, src/query/weight.rs:23-35,101-121, src/collector/mod.rs:186-221)
// as CSR rows of ascending doc ids.  Every list is reached through bitmap words: its own bitmap, or — a list without
// one — bits scattered into the batch's scratch (count_scatter_kernel); tq_docset.hip counts, scans and writes.
// tq_docset_scored_batch*: the same rows with every doc's BM25 score (Weight::for_each, src/query/weight.rs:9-18,89-97):
// tq_docset_score.hip's pass behind every write pass, over a scoring descriptor of its own (score_expression).
// Options "docset_trees" / "docset_score_trees" (unscored / scored calls): a phrase or a nested boolean query is planned by
// plan_tree_query — scored: from the caller's weights, its tf_cache joining the batch's cache blob — its exact match bits
// are written into ONE slot of the same scratch by tq_docset_tree.hip behind the sub-batch's scatter, and the passes see
// one Must list that is bits in scratch; tq_docset_tree_score.hip scores its rows next to the flat pass.  The lists' tables
// (their own or the probe pool's) live for the whole call; only the result bits are the sub-batch's, and the scoring pass
// does not read them.
// docset_batch runs one DocsetCall as stages around one Batch record: check_and_express, plan_trees, cut_docset_subs,
// size_and_upload, then per sub-batch launch_match_bits and launch_consumer, driven by run_device / run_host.  The consumer
// of a sub-batch's match words is one of four: rows, the count pass alone (tq_count_batch), or the launches tq_sort.cpp
// (tq_search_sorted_batch*) / tq_agg.cpp (tq_agg_batch*, tq_agg_sub_batch*, tq_agg_terms_batch*, tq_agg_terms_sub_batch*, tq_agg_range_batch*, tq_agg_terms_hist_batch*) put in place of the count / scan / write passes.
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
  if (fc.empty_set()) {
    dq.min_should = 1;  // no lists, one Should clause wanted: the empty set
    return FLAT_OK;
  }
  const bool should_is_must = fc.should_is_must();
  const uint32_t msm = should_is_must ? 0u : fc.msm;
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
  if (fc.empty_set()) return;
  const bool should_is_must = fc.should_is_must();
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

void cut_docset_subs(const tq_segment *s, std::vector<TqkDocsetQuery> &dqs, const std::vector<TqkScoreQuery> &sqs,
                     const std::vector<uint32_t> &tree_q, std::vector<TqdTreeQuery> &tqs, const std::vector<uint32_t> &slop_qi,
                     std::vector<TqdSlopQuery> &slop_qs, uint32_t max_temp, uint32_t max_sub_queries, DocsetCut &cut) {
  const uint32_t n_queries = (uint32_t)dqs.size();
  std::vector<uint4> &wgs = cut.wgs;
  std::unordered_map<uint32_t, uint32_t> slot;  // a list without a bitmap gets a slot of the scratch for the duration of its sub-batch
  DocsetSubBatch cur;
  uint32_t n_slots = 0;  // slots of the sub-batch so far: its lists without a bitmap, its trees' and sloppy phrases' results
  uint32_t n_trees = 0;  // tree queries so far
  uint32_t n_slops = 0;  // sloppy phrases so far
  auto close_sub = [&](uint32_t q1) {
    cur.q1 = q1;
    cur.wg1 = wgs.size();
    cur.t1 = n_trees;
    cur.s1 = n_slops;
    cur.n_temp = n_slots;
    for (uint32_t qi = cur.q0; qi < q1 && qi < sqs.size(); ++qi)
      for (uint32_t m = 0; m < sqs[qi].n_lists; ++m)
        cur.score_blocks = cur.score_blocks || ((sqs[qi].access >> (2u * m)) & 3u) == TQK_SCORE_BLOCKS;
    cut.max_sub_temp = std::max(cut.max_sub_temp, cur.n_temp);
    cut.max_sub_n = std::max(cut.max_sub_n, cur.q1 - cur.q0);
    cut.subs.push_back(cur);
    cur = DocsetSubBatch{};
    cur.q0 = q1;
    cur.wg0 = wgs.size();
    cur.t0 = n_trees;
    cur.s0 = n_slops;
    slot.clear();
    n_slots = 0;
  };
  for (uint32_t qi = 0; qi < n_queries; ++qi) {
    TqkDocsetQuery &dq = dqs[qi];
    const bool tree = n_trees < tree_q.size() && tree_q[n_trees] == qi;
    if (tree || (n_slops < slop_qi.size() && slop_qi[n_slops] == qi)) {  // one result slot, like a fresh list
      if (qi > cur.q0 && (n_slots + 1u > max_temp || qi - cur.q0 >= max_sub_queries)) close_sub(qi);
      if (tree) cur.any_phrase = cur.any_phrase || tqs[n_trees].has_phrase;
      (tree ? tqs[n_trees++].part_start : slop_qs[n_slops++].part_start) = n_slots;
      dq.dense[0] = (const uint2 *)(uintptr_t)n_slots++;  // (the slot; the pointer once the scratch is sized)
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
        push_scatter_work(wgs, s, h, it->second);
      }
      dq.dense[m] = (const uint2 *)(uintptr_t)it->second;  // (the slot)
    }
  }
  if (n_queries) close_sub(n_queries);
}

namespace {

using Consumer = DocsetConsumer;
enum : uint32_t { DS_SCATTER = 1u, DS_COUNT = 2u, DS_WRITE = 4u };

// What one batch carries from stage to stage.
struct Batch {
  tq_segment *s;  // the call
  const tq_query *queries;
  uint32_t n_queries;
  const DocsetCall &call;
  hipStream_t st = nullptr;
  // the geometry: bitmap words per list (in scratch: padded), tiles, and what one sub-batch may take of slots and queries
  uint32_t n_words = 0, words_per_list = 0, n_tiles = 0, max_temp = 0, max_sub_queries = 1;
  std::vector<TqkDocsetQuery> dqs;    // check_and_express: every query's expression (a tree's, a sloppy phrase's: plan_trees)
  std::vector<TqkScoreQuery> sqs;     // ... and, in a scored call, its scoring lists
  std::vector<const float *> caches;  // the batch's Bm25Weight caches in order of first use (pointer identity, as in search)
  bool score_fields = false;          // some scoring list of the batch belongs to a non-primary field
  uint64_t algo_bytes = 0;
  std::vector<uint32_t> tree_q;  // the queries that take the tree path, ascending
  // Sloppy phrases (tq_phrase_slop.cpp), ascending, and their views: the existence verdict of the reference's non-scoring
  // PhraseScorer as match bits in a result slot of their own, like a tree's.
  std::vector<uint32_t> slop_qi;
  std::deque<SlopView> slop_views;
  std::vector<TqdTreeQuery> tqs;  // plan_trees: the records of tree_q and slop_qi, in their order
  std::vector<TqdSlopQuery> slop_qs;
  DocsetCut cut;
  // size_and_upload: where the trees' query map and the sloppy phrases' records stand in d_docset_trees; the timing ring;
  // the row starts on the device (the caller's array, or the host variant's scratch)
  size_t tree_bytes = 0, slop_off = 0;
  bool timed = false;
  int ring = 0;
  uint64_t *d_starts = nullptr;

  // (what the call says about a sloppy phrase — refusals, the overflow words — it says under the CALLER's index)
  uint32_t named(uint32_t qi) const { return call.caller_q ? call.caller_q[qi] : qi; }
  uint32_t n_over_words() const { return call.caller_q ? call.n_caller : n_queries; }
  bool own_passes() const { return call.consumer == Consumer::kRows || call.consumer == Consumer::kCount; }
  // (a multi-field segment: tf_cache is one row per field, the rows go up together and the index names row 0)
  uint32_t cache_index(const float *tc) {
    const uint32_t rows = s->n_fields;
    for (size_t ci = caches.size(); ci >= rows; ci -= rows)  // (last first: neighbours share one)
      if (caches[ci - rows] == tc) return (uint32_t)(ci - rows);
    for (uint32_t f = 0; f < rows; ++f) caches.push_back(tc + (size_t)f * 256u);
    return (uint32_t)(caches.size() - rows);
  }
};

// the scored calls' rule: weights and a tf_cache, the first n weights finite
int check_weights(const char *fn, uint32_t qi, const tq_query &q, uint32_t n) {
  if (!q.weights || !q.tf_cache) return fail(TQ_ERR_INVALID, "%s: query %u: null weights / tf_cache", fn, qi);
  for (uint32_t i = 0; i < n; ++i)
    if (!std::isfinite(q.weights[i])) return fail(TQ_ERR_INVALID, "%s: query %u: weight %u is not finite", fn, qi, i);
  return TQ_OK;
}

// Every query is checked, in index order, before anything is launched — a batch fails as a whole — and sorted into flat
// (its expressions), tree or sloppy.
int check_and_express(Batch &b) {
  tq_segment *const s = b.s;
  const char *const fn = b.call.fn;
  const bool scored = b.call.scored, count_only = b.call.consumer == Consumer::kCount;
  const bool trees_on = count_only ? false : scored ? s->opt.docset_score_trees != 0 : s->opt.docset_trees != 0;
  const bool fields = s->n_field_terms != 0;  // (0: no query is looked at for fields)
  for (uint32_t qi = 0; qi < b.n_queries; ++qi) {
    const char *why = "";
    FlatClauses fc;
    const tq_query &q = b.queries[qi];
    if (q.slop) {
      b.slop_views.emplace_back();
      const int vrc = slop_view(s, q, b.named(qi), fn, b.slop_views.back(), false);
      if (vrc != TQ_OK) return vrc;
      if (scored)
        return fail(TQ_ERR_UNSUPPORTED, "%s: query %u: scored doc sets of sloppy phrases stay on the CPU in this version", fn, b.named(qi));
      if (!trees_on && !count_only)
        return fail(TQ_ERR_UNSUPPORTED, "%s: query %u is a phrase: doc sets of phrases and nested queries stay on the CPU (option \"docset_trees\")", fn, b.named(qi));
      b.slop_qi.push_back(qi);
      continue;
    }
    bool names_set = false;  // a term set in a phrase, inside a nested query, or released: refused whatever the tree options say
    const int src = check_set_query(s, q, qi, fn, &names_set);
    if (src != TQ_OK) return src;
    const bool names_field = fields && query_names_field(s, q);
    if (names_field) {  // a phrase over two fields: refused whatever the tree options say
      const int frc = check_field_query(s, q, qi, fn);
      if (frc != TQ_OK) return frc;
    }
    const int rc = docset_expression(s, q, b.dqs[qi], &why, scored ? &fc : nullptr);
    if (rc == FLAT_UNSUPPORTED && trees_on && !query_has_all(q) && (q.mode == TQ_MODE_PHRASE || bool_query_is_tree(q))) {
      if (scored && names_field)  // (docset_tree_score_kernel scores under the primary field's norms)
        return fail(TQ_ERR_UNSUPPORTED, "%s: query %u: scored doc sets of phrases and nested queries that name a non-primary field stay on the CPU in this version", fn, qi);
      if (scored) {  // plan_tree_query reads every term's weight (a phrase: its first)
        const int wrc = check_weights(fn, qi, q, q.mode == TQ_MODE_PHRASE ? std::min(q.n_terms, 1u) : q.n_terms);
        if (wrc != TQ_OK) return wrc;
      }
      b.tree_q.push_back(qi);
      continue;
    }
    if (rc == FLAT_UNSUPPORTED)
      return fail(TQ_ERR_UNSUPPORTED, "%s: query %u is %s: doc sets of phrases and nested queries stay on the CPU", fn, qi, why);
    if (rc != FLAT_OK) return fail(TQ_ERR_INVALID, "%s: query %u: %s", fn, qi, why);
    b.algo_bytes += (uint64_t)b.dqs[qi].n_terms * b.n_words * 4u;
    if (!scored) continue;
    bool has_list = false;
    for (uint32_t c = 0; c < fc.n_cl; ++c) has_list = has_list || (fc.cl[c].occur != TQ_MUST_NOT && fc.cl[c].n);
    if (has_list) {
      const int wrc = check_weights(fn, qi, q, q.n_terms);
      if (wrc != TQ_OK) return wrc;
    }
    if (fc.all_boost_mixed)
      return fail(TQ_ERR_UNSUPPORTED, "%s: query %u has a boosted match-all clause beside another scoring clause or a second match-all clause: its scores stay on the CPU",
                  fn, qi);
    TqkScoreQuery &sq = b.sqs[qi];
    if (has_list || fc.all_based) score_expression(s, q, fc, sq);
    if (sq.n_lists) sq.cache_idx = b.cache_index(q.tf_cache);
    for (uint32_t m = 0; names_field && m < sq.n_lists; ++m) b.score_fields = b.score_fields || (sq.shift[m] >> 8) != 0u;
    b.algo_bytes += (uint64_t)sq.n_lists * b.n_words * 8u;
  }
  return TQ_OK;
}

// to the passes a tree or a sloppy phrase is one Must list that is bits in scratch
void one_scratch_list(TqkDocsetQuery &dq) {
  dq = TqkDocsetQuery{};
  dq.n_terms = dq.narrow = dq.clause_end = 1u;
}

// The batch's trees and sloppy phrases: every list of theirs as a bitmap + tf bytes, a phrase term's position directory —
// the list's own tables or the probe pool's, built now in a probe batch like a search batch's, so that no list of this
// call is evicted for another — then their records, and what they read in the byte model.
int plan_trees(Batch &b) {
  if (b.tree_q.empty() && b.slop_qi.empty()) return TQ_OK;
  tq_segment *const s = b.s;
  const bool scored = b.call.scored;
  probe_begin_batch(s);
  std::deque<TreeView> views;
  bool built = false;
  for (const uint32_t qi : b.tree_q) {
    views.emplace_back();
    docset_tree_view(b.queries[qi], views.back(), scored);
    const int prc = build_tree_query_probe_tables(s, views.back().q, &built);
    if (prc != TQ_OK) return prc;
  }
  for (const SlopView &sv : b.slop_views) {
    const int prc = build_tree_query_probe_tables(s, sv.v.q, &built);
    if (prc != TQ_OK) return prc;
  }
  if (built) s->share_span_terms = ~(size_t)0;
  update_table_span(s);
  if (!s->share_span_ok || !s->opt.use_dense)
    return fail_tree_tables(s, b.named(std::min(b.tree_q.empty() ? ~0u : b.tree_q[0], b.slop_qi.empty() ? ~0u : b.slop_qi[0])));
  b.tqs.resize(b.tree_q.size());
  b.slop_qs.resize(b.slop_qi.size());
  for (size_t k = 0; k < b.slop_qi.size(); ++k) {
    // (named: the query in refusals, and its overflow word; the lists' bits once + the result word written and read back)
    const uint32_t qi = b.slop_qi[k];
    const int prc = plan_slop_query(s, b.slop_views[k].v.q, b.named(qi), b.queries[qi].slop, b.slop_qs[k], b.algo_bytes, true);
    if (prc != TQ_OK) return prc;
    one_scratch_list(b.dqs[qi]);
  }
  for (size_t i = 0; i < b.tree_q.size(); ++i) {
    TqdTreeQuery &tq = b.tqs[i];
    uint64_t qbytes = 0;
    const int prc = plan_tree_query(s, views[i].q, b.tree_q[i], tq, qbytes, s->share_table_lo);
    if (prc != TQ_OK) return prc;  // (names the query)
    one_scratch_list(b.dqs[b.tree_q[i]]);
    // every list's bits once + the result word written and read back
    b.algo_bytes += ((uint64_t)tq.n_terms + 2u) * b.n_words * 4u;
    if (!scored) continue;
    // its cache in the blob the flat queries use: one index space for both scoring kernels
    if (tq.n_terms) tq.cache_idx = b.cache_index(b.queries[b.tree_q[i]].tf_cache);
    // the scoring pass: one bitmap word per 32 docs for every list that scores (under no MustNot on either level)
    uint32_t n_scoring = 0;
    for (uint32_t c = 0; c < tq.n_clauses; ++c)
      for (uint32_t t = tq.first_term[c]; t < tq.first_term[c + 1u]; ++t)
        n_scoring += tq.outer[c] != TQ_MUST_NOT && tq.inner[t] != TQ_MUST_NOT ? 1u : 0u;
    b.algo_bytes += (uint64_t)n_scoring * b.n_words * 8u;
  }
  return TQ_OK;
}

// The batch's scratch sized, the slots of lists without a bitmap turned into pointers, and everything the launches read
// on its way up through one staging blob [dqs | work list | sqs | caches | tqs | their query map | slop_qs].
int size_and_upload(Batch &b) {
  tq_segment *const s = b.s;
  const DocsetCall &call = b.call;
  const bool scored = call.scored;
  const uint32_t n_queries = b.n_queries;
  hipStream_t st = b.st;
  const size_t q_bytes = (size_t)n_queries * sizeof(TqkDocsetQuery), wg_bytes = b.cut.wgs.size() * sizeof(uint4);
  const size_t sq_bytes = b.sqs.size() * sizeof(TqkScoreQuery), cache_bytes = b.caches.size() * 256u * sizeof(float);
  b.tree_bytes = b.tqs.size() * sizeof(TqdTreeQuery);
  // scored: behind the records, which query of its sub-batch every tree is (tq_docset_tree_score.hip: tile_counts / tile_offs)
  static_assert(sizeof(TqdTreeQuery) % sizeof(uint32_t) == 0, "the map stands right behind the records");
  const size_t tree_map_bytes = scored ? b.tqs.size() * sizeof(uint32_t) : 0u;
  const size_t max_entries = (size_t)b.cut.max_sub_n * b.n_tiles;
  // (the sloppy phrases' records ride behind the tree records and their map, 64-byte aligned, in both buffers)
  const size_t slop_bytes = b.slop_qs.size() * sizeof(TqdSlopQuery);
  b.slop_off = (b.tree_bytes + tree_map_bytes + 63u) & ~(size_t)63;
  const size_t tree_blob_bytes = slop_bytes ? b.slop_off + slop_bytes : b.tree_bytes + tree_map_bytes;
  const size_t tree_at = q_bytes + wg_bytes + sq_bytes + cache_bytes;
  int rc = s->h_docset.ensure(tree_at + tree_blob_bytes + 64u);
  if (rc == TQ_OK && tree_blob_bytes) rc = s->d_docset_trees.ensure(tree_blob_bytes);
  if (rc == TQ_OK && slop_bytes) rc = s->d_slop_over.ensure((size_t)b.n_over_words() * sizeof(uint32_t));
  if (rc == TQ_OK && scored) rc = s->d_docset_squeries.ensure(sq_bytes);
  if (rc == TQ_OK && scored) rc = s->d_docset_caches.ensure(std::max<size_t>(cache_bytes, 256u * sizeof(float)));
  if (rc == TQ_OK) rc = s->d_docset_queries.ensure(q_bytes);
  if (rc == TQ_OK) rc = s->d_count_wgs.ensure(wg_bytes);
  if (rc == TQ_OK) rc = s->d_count_bits.ensure((size_t)b.cut.max_sub_temp * b.words_per_list * sizeof(uint32_t));
  if (rc == TQ_OK && b.own_passes()) rc = s->d_docset_counts.ensure(max_entries * sizeof(uint32_t));
  if (rc == TQ_OK && b.own_passes()) rc = s->d_docset_offs.ensure(max_entries * sizeof(uint64_t));
  if (rc == TQ_OK && b.own_passes()) rc = s->d_docset_partials.ensure(((max_entries + tqk_docset_scan_tile() - 1) / tqk_docset_scan_tile()) * sizeof(uint64_t));
  if (rc == TQ_OK) rc = s->d_qmatches.ensure((size_t)n_queries * sizeof(uint32_t));
  if (rc == TQ_OK && !call.device_out) rc = s->d_docset_starts.ensure(((size_t)n_queries + 1u) * sizeof(uint64_t));
  if (rc != TQ_OK) return rc;
  b.d_starts = call.device_out ? call.out_starts : (uint64_t *)s->d_docset_starts.p;
  for (TqkDocsetQuery &dq : b.dqs)
    for (uint32_t m = 0; m < dq.n_terms; ++m)
      if ((dq.narrow >> m) & 1u)
        dq.dense[m] = (const uint2 *)((const uint32_t *)s->d_count_bits.p + (size_t)(uintptr_t)dq.dense[m] * b.words_per_list);
  // option "timing" (device variant): the batch takes a slot of the event ring like a search batch
  b.timed = call.device_out && s->opt.timing;
  b.ring = (int)(s->batches_timed % tq_segment::kTimingRing);
  if (b.timed) HIP_TRY(hipEventRecord(s->ev_t0[b.ring], st));
  uint8_t *const h = (uint8_t *)s->h_docset.p;
  memcpy(h, b.dqs.data(), q_bytes);
  if (wg_bytes) memcpy(h + q_bytes, b.cut.wgs.data(), wg_bytes);
  HIP_TRY(hipMemcpyAsync(s->d_docset_queries.p, h, q_bytes, hipMemcpyHostToDevice, st));
  if (wg_bytes) HIP_TRY(hipMemcpyAsync(s->d_count_wgs.p, h + q_bytes, wg_bytes, hipMemcpyHostToDevice, st));
  if (scored) {
    uint8_t *const h_sq = h + q_bytes + wg_bytes;
    memcpy(h_sq, b.sqs.data(), sq_bytes);
    for (size_t c = 0; c < b.caches.size(); ++c) memcpy(h_sq + sq_bytes + c * 256u * sizeof(float), b.caches[c], 256u * sizeof(float));
    HIP_TRY(hipMemcpyAsync(s->d_docset_squeries.p, h_sq, sq_bytes, hipMemcpyHostToDevice, st));
    if (cache_bytes) HIP_TRY(hipMemcpyAsync(s->d_docset_caches.p, h_sq + sq_bytes, cache_bytes, hipMemcpyHostToDevice, st));
  }
  if (tree_blob_bytes) {
    uint8_t *const h_tq = h + tree_at;
    if (b.tree_bytes) memcpy(h_tq, b.tqs.data(), b.tree_bytes);
    if (tree_map_bytes) {
      uint32_t *const map = (uint32_t *)(h_tq + b.tree_bytes);
      for (const DocsetSubBatch &sb : b.cut.subs)
        for (uint32_t t = sb.t0; t < sb.t1; ++t) map[t] = b.tree_q[t] - sb.q0;
    }
    if (slop_bytes) memcpy(h_tq + b.slop_off, b.slop_qs.data(), slop_bytes);
    HIP_TRY(hipMemcpyAsync(s->d_docset_trees.p, h_tq, tree_blob_bytes, hipMemcpyHostToDevice, st));
  }
  if (call.consumer == Consumer::kSort) rc = sort_prepare(s, *call.sort, b.queries, n_queries, b.cut.max_sub_n, b.n_words, st);
  if (call.consumer == Consumer::kAgg) rc = agg_prepare(s, *call.agg, n_queries, b.cut.max_sub_n, b.n_words, st);
  if (rc != TQ_OK) return rc;
  if (slop_bytes) {  // the overflow words, one per query of the batch (tq_last_batch_slop_overflows)
    HIP_TRY(hipMemsetAsync(s->d_slop_over.p, 0, (size_t)b.n_over_words() * sizeof(uint32_t), st));
    s->last_batch_slop = true;
  }
  return TQ_OK;
}

// The match bits a sub-batch's passes read from scratch: its lists without a bitmap scattered, its trees and its sloppy
// phrases evaluated — every word of a result slot is stored, once.
int launch_match_bits(const Batch &b, const DocsetSubBatch &sb) {
  tq_segment *const s = b.s;
  if (sb.wg1 > sb.wg0) {
    HIP_TRY(hipMemsetAsync(s->d_count_bits.p, 0, (size_t)sb.n_temp * b.words_per_list * sizeof(uint32_t), b.st));
    const int rc = launched(tqk_launch_count_scatter(s->dseg, s->d_terms, (const uint4 *)s->d_count_wgs.p + sb.wg0, (uint32_t)(sb.wg1 - sb.wg0),
                                                     (uint32_t *)s->d_count_bits.p, b.words_per_list, b.st), "doc-set scatter");
    if (rc != TQ_OK) return rc;
  }
  if (sb.t1 > sb.t0) {
    TqkDocsetTreeParams tp{};
    tp.seg = s->dseg;
    tp.terms = s->d_terms;
    tp.queries = (const TqdTreeQuery *)s->d_docset_trees.p + sb.t0;
    tp.table_base = (const uint8_t *)s->share_table_lo;
    tp.bits = (uint32_t *)s->d_count_bits.p;
    tp.n_queries = sb.t1 - sb.t0;
    tp.n_words = b.n_words;
    tp.words_per_list = b.words_per_list;
    tp.any_phrase = sb.any_phrase ? 1u : 0u;
    const int rc = launched(tqk_launch_docset_tree(tp, b.st), "doc-set tree");
    if (rc != TQ_OK) return rc;
  }
  if (sb.s1 > sb.s0) {
    TqkPhraseSlopParams pp{};
    pp.seg = s->dseg;
    pp.terms = s->d_terms;
    pp.queries = (const TqdSlopQuery *)((const uint8_t *)s->d_docset_trees.p + b.slop_off) + sb.s0;
    pp.table_base = (const uint8_t *)s->share_table_lo;
    pp.overflow = (uint32_t *)s->d_slop_over.p;
    pp.bits = (uint32_t *)s->d_count_bits.p;
    pp.n_queries = sb.s1 - sb.s0;
    pp.n_words = b.n_words;
    pp.words_per_list = b.words_per_list;
    for (uint32_t k = sb.s0; k < sb.s1; ++k) (b.slop_qs[k].n_terms > 2u ? pp.any_carry : pp.any_pair) = 1u;
    return launched(tqk_launch_phrase_slop_bits(pp, b.st), "sloppy phrase");
  }
  return TQ_OK;
}

// The scoring passes right behind a sub-batch's write pass (p: that pass's parameters; the tables are this sub-batch's).
hipError_t launch_scores(const Batch &b, const DocsetSubBatch &sb, const TqkDocsetParams &p, float *d_scores) {
  tq_segment *const s = b.s;
  TqkScoreParams sp{};
  sp.seg = s->dseg;
  sp.terms = s->d_terms;
  sp.caches = (const float *)s->d_docset_caches.p;
  sp.out_docs = p.out_docs;
  sp.out_scores = d_scores;
  sp.out_cap = p.out_cap;
  sp.n_tiles = b.n_tiles;
  sp.any_blocks = sb.score_blocks ? 1u : 0u;
  // the flat pass over the runs of flat queries between the sub-batch's trees (no tree: one launch): a tree's row is
  // the tree pass's alone — the flat kernel would store the empty sum over it
  hipError_t e = hipSuccess;
  uint32_t r0 = sb.q0;
  for (uint32_t t = sb.t0; t <= sb.t1 && e == hipSuccess; ++t) {
    const uint32_t r1 = t < sb.t1 ? b.tree_q[t] : sb.q1;
    if (r1 > r0) {
      sp.queries = (const TqkScoreQuery *)s->d_docset_squeries.p + r0;
      sp.tile_counts = p.tile_counts + (size_t)(r0 - sb.q0) * b.n_tiles;
      sp.tile_offs = p.tile_offs + (size_t)(r0 - sb.q0) * b.n_tiles;
      sp.n_queries = r1 - r0;
      if (b.score_fields) {  // per-list norms (tq_fields.cpp)
        TqkScoreFieldsParams fp{};
        fp.base = sp;
        fp.fn[0] = s->d_fn;
        for (uint32_t f = 1; f < TQK_MAX_FIELDS; ++f) fp.fn[f] = s->d_fn_field[f];
        e = tqk_launch_docset_score_fields(fp, b.st);
      } else {
        e = tqk_launch_docset_score(sp, b.st);
      }
    }
    r0 = r1 + 1u;
  }
  if (e != hipSuccess || sb.t1 == sb.t0) return e;
  TqkDocsetTreeScoreParams tsp{};
  tsp.seg = s->dseg;
  tsp.terms = s->d_terms;
  tsp.queries = (const TqdTreeQuery *)s->d_docset_trees.p + sb.t0;
  tsp.query_of = (const uint32_t *)((const uint8_t *)s->d_docset_trees.p + b.tree_bytes) + sb.t0;
  tsp.caches = sp.caches;
  tsp.table_base = (const uint8_t *)s->share_table_lo;
  tsp.tile_counts = p.tile_counts;
  tsp.tile_offs = p.tile_offs;
  tsp.out_docs = p.out_docs;
  tsp.out_scores = d_scores;
  tsp.out_cap = p.out_cap;
  tsp.n_queries = sb.t1 - sb.t0;
  tsp.n_tiles = b.n_tiles;
  tsp.any_phrase = sb.any_phrase ? 1u : 0u;
  return tqk_launch_docset_tree_score(tsp, b.st);
}

// What consumes a sub-batch's match words: the count / scan / write (and scoring) passes `stages` names, or the sort's or
// the aggregation's launches in their place.
int launch_consumer(const Batch &b, const DocsetSubBatch &sb, uint32_t stages, uint32_t *d_docs, float *d_scores, uint64_t cap) {
  // the write pass stages the docs of a (query, tile) in LDS when the tile holds at least this many (of 65 536)
  static const uint32_t kStageMin = tune_u32("TQ_DOCSET_STAGE_MIN", 2048);
  tq_segment *const s = b.s;
  TqkDocsetParams p{};
  p.queries = (const TqkDocsetQuery *)s->d_docset_queries.p + sb.q0;
  p.alive = s->d_alive;
  p.tile_counts = (uint32_t *)s->d_docset_counts.p;
  p.tile_offs = (uint64_t *)s->d_docset_offs.p;
  p.partials = (uint64_t *)s->d_docset_partials.p;
  p.base_in = sb.q0 ? b.d_starts + sb.q0 : nullptr;  // (the total the sub-batch before left there)
  p.out_starts = b.d_starts + sb.q0;
  p.query_sizes = (uint32_t *)s->d_qmatches.p + sb.q0;
  p.total_out = s->d_match_counter;
  p.out_docs = d_docs;
  p.out_cap = cap;
  p.n_queries = sb.q1 - sb.q0;
  p.n_tiles = b.n_tiles;
  p.n_words = b.n_words;
  p.max_doc = s->max_doc;
  p.stage_min_docs = kStageMin;
  if (b.call.consumer == Consumer::kSort) return sort_launch(s, *b.call.sort, p, sb.q0, b.st);
  if (b.call.consumer == Consumer::kAgg) return agg_launch(s, *b.call.agg, p, sb.q0, b.st);
  hipError_t e = hipSuccess;
  if (stages & DS_COUNT) {
    e = tqk_launch_docset_count(p, b.st);
    if (e == hipSuccess) e = tqk_launch_docset_scan(p, b.st);
  }
  if (e == hipSuccess && (stages & DS_WRITE)) e = tqk_launch_docset_write(p, b.st);
  if (e == hipSuccess && (stages & DS_WRITE) && b.call.scored) e = launch_scores(b, sb, p, d_scores);
  return launched(e, "doc-set kernel");
}

int sweep(const Batch &b, uint32_t stages, uint32_t *d_docs, float *d_scores, uint64_t cap) {
  for (const DocsetSubBatch &sb : b.cut.subs) {
    int rc = (stages & DS_SCATTER) ? launch_match_bits(b, sb) : TQ_OK;
    if (rc == TQ_OK) rc = launch_consumer(b, sb, stages, d_docs, d_scores, cap);
    if (rc != TQ_OK) return rc;
  }
  return TQ_OK;
}

// Device outputs: one sweep, enqueued; the total stays on the device (tq_last_batch_stats reads it).
int run_device(const Batch &b) {
  tq_segment *const s = b.s;
  const DocsetCall &call = b.call;
  if (b.timed) HIP_TRY(hipEventRecord(s->ev_k0[b.ring], b.st));
  int rc = sweep(b, DS_SCATTER | DS_COUNT | DS_WRITE, call.out_docs, call.out_scores, call.out_cap);
  if (rc == TQ_OK && call.consumer == Consumer::kAgg) rc = agg_finish(s, *call.agg, b.n_queries, b.st);
  if (rc != TQ_OK) return rc;
  if (b.timed) {
    HIP_TRY(hipEventRecord(s->ev_k1[b.ring], b.st));
    HIP_TRY(hipEventRecord(s->ev_t1[b.ring], b.st));
    ++s->batches_timed;
  }
  s->stats_pending = true;
  s->stats_match_bytes = call.scored ? 9 : 4;  // doc [+ score + fieldnorm byte]
  s->stats_sorted = !b.own_passes();           // (its own byte model: tq_last_batch_stats)
  s->stats_sorted_optional = (call.sort && call.sort->optional) || (call.agg && call.agg->optional);
  s->stats_agg_metric = call.agg && call.agg->metric;
  s->stats_agg_metric_optional = call.agg && call.agg->metric_optional;
  s->stats_agg_terms = call.agg && call.agg->terms;
  s->stats_agg_terms_sub = call.agg && call.agg->terms_sub;
  s->stats_agg_terms_hist_row = call.agg && call.agg->terms_hist ? call.agg->plan.n_buckets + 1u : 0u;
  HIP_TRY(hipEventRecord(s->ev_batch_done, b.st));
  s->last_stream = b.st;
  s->batch_in_flight = true;
  return TQ_OK;
}

// Host outputs: the count sweep and the row starts first — they say whether the docs fit — then the write sweep and the
// copy back.  The call waits for the device anyway: a sloppy phrase whose carried list went over the cap is reported
// last, the rows of the other queries are written and valid.
int run_host(const Batch &b) {
  tq_segment *const s = b.s;
  const DocsetCall &call = b.call;
  const std::vector<DocsetSubBatch> &subs = b.cut.subs;
  int rc = sweep(b, DS_SCATTER | DS_COUNT, nullptr, nullptr, 0);
  if (rc != TQ_OK) return rc;
  HIP_TRY(hipMemcpyAsync(call.out_starts, b.d_starts, ((size_t)b.n_queries + 1u) * sizeof(uint64_t), hipMemcpyDeviceToHost, b.st));
  HIP_TRY(hipStreamSynchronize(b.st));
  const uint64_t total = call.out_starts[b.n_queries];
  s->stats.matches = total;
  if (call.consumer == Consumer::kCount) return slop_overflow_readback(s, call.fn);  // (the row starts are the counts)
  s->stats.algorithmic_bytes += (call.scored ? 9u : 4u) * total;
  if (total > call.out_cap)
    return fail(TQ_ERR_INVALID, "%s: the batch has %llu docs, out_cap is %llu (out_starts is filled: retry with that many)", call.fn,
                (unsigned long long)total, (unsigned long long)call.out_cap);
  if (!total) return slop_overflow_readback(s, call.fn);
  rc = s->d_docset_docs.ensure((size_t)total * sizeof(uint32_t));
  if (rc == TQ_OK && call.scored) rc = s->d_docset_scores.ensure((size_t)total * sizeof(float));
  if (rc != TQ_OK) return rc;
  // one sub-batch: its tables and bits are still there, positions are walked once; several: each is evaluated again (the
  // scratch held the last one's), and the overflow words count every candidate once
  if (subs.size() > 1 && !b.slop_qs.empty())
    HIP_TRY(hipMemsetAsync(s->d_slop_over.p, 0, (size_t)b.n_over_words() * sizeof(uint32_t), b.st));
  rc = sweep(b, subs.size() == 1 ? DS_WRITE : (DS_SCATTER | DS_COUNT | DS_WRITE), (uint32_t *)s->d_docset_docs.p, (float *)s->d_docset_scores.p, total);
  if (rc != TQ_OK) return rc;
  HIP_TRY(hipMemcpyAsync(call.out_docs, s->d_docset_docs.p, (size_t)total * sizeof(uint32_t), hipMemcpyDeviceToHost, b.st));
  if (call.scored) HIP_TRY(hipMemcpyAsync(call.out_scores, s->d_docset_scores.p, (size_t)total * sizeof(float), hipMemcpyDeviceToHost, b.st));
  HIP_TRY(hipStreamSynchronize(b.st));
  if (s->d_docset_docs.cap > ((size_t)256 << 20)) s->d_docset_docs.release();  // (a large result is not kept as scratch)
  if (s->d_docset_scores.cap > ((size_t)256 << 20)) s->d_docset_scores.release();
  return slop_overflow_readback(s, call.fn);
}

}  // namespace

int docset_batch(tq_segment *s, const tq_query *queries, uint32_t n_queries, const DocsetCall &call) {
  static const uint64_t kTempBudget = (uint64_t)std::max<uint32_t>(1u, tune_u32("TQ_COUNT_TEMP_MB", 1024)) << 20;
  Batch b{s, queries, n_queries, call};
  b.n_words = (uint32_t)(((uint64_t)s->max_doc + 31u) / 32u);
  b.words_per_list = (b.n_words + 63u) & ~63u;
  b.n_tiles = (b.n_words + tqk_docset_tile_words() - 1u) / tqk_docset_tile_words();
  b.max_temp = s->opt.docset_temp_lists > 0
                   ? (uint32_t)s->opt.docset_temp_lists
                   : (uint32_t)std::min<uint64_t>(4096u, kTempBudget / std::max<uint64_t>(1u, (uint64_t)b.words_per_list * 4u));
  b.max_temp = std::max<uint32_t>(b.max_temp, TQ_MAX_TERMS);  // a single query always fits
  b.max_sub_queries = std::max<uint32_t>(1u, (1u << 26) / std::max(1u, b.n_tiles));
  b.dqs.resize(n_queries);
  b.sqs.resize(call.scored ? n_queries : 0u);
  s->last_batch_slop = false;
  s->slop_over_words = b.n_over_words();
  int rc = check_and_express(b);
  if (rc == TQ_OK) rc = plan_trees(b);  // (planning errors come after every per-query check)
  if (rc != TQ_OK) return rc;
  cut_docset_subs(s, b.dqs, b.sqs, b.tree_q, b.tqs, b.slop_qi, b.slop_qs, b.max_temp, b.max_sub_queries, b.cut);

  HIP_TRY(hipSetDevice(s->device));
  b.st = call.device_out && call.hip_stream ? (hipStream_t)call.hip_stream : s->stream;
  rc = wait_segment_idle(s);  // the scratch below is shared with the batches before
  if (rc != TQ_OK) return rc;
  const bool scored = call.scored;
  s->stats = tq_batch_stats{};
  s->stats.kernel_mask = (call.consumer == Consumer::kSort ? TQ_KERNEL_SORT : call.consumer == Consumer::kAgg ? (call.agg->terms_hist ? TQ_KERNEL_AGG_TERMS_HIST : call.agg->terms_sub ? TQ_KERNEL_AGG_TERMS_SUB : call.agg->terms ? TQ_KERNEL_AGG_TERMS : call.agg->range ? TQ_KERNEL_AGG_RANGE : call.agg->metric ? TQ_KERNEL_AGG_SUB : TQ_KERNEL_AGG) : TQ_KERNEL_DOCSET) |
                         (scored ? TQ_KERNEL_DOCSET_SCORE : 0u) | (b.tqs.empty() ? 0u : TQ_KERNEL_DOCSET_TREE) |
                         (scored && !b.tqs.empty() ? TQ_KERNEL_DOCSET_TREE_SCORE : 0u) | (b.slop_qs.empty() ? 0u : TQ_KERNEL_PHRASE_SLOP);
  s->stats.algorithmic_bytes = b.algo_bytes;
  s->stats_pending = false;
  s->last_batch_queries = 0;
  if (b.own_passes() && (n_queries == 0 || b.n_tiles == 0)) {  // no query, or a segment without docs: empty rows
    if (call.device_out) {
      HIP_TRY(hipMemsetAsync(call.out_starts, 0, ((size_t)n_queries + 1u) * sizeof(uint64_t), b.st));
    } else {
      memset(call.out_starts, 0, ((size_t)n_queries + 1u) * sizeof(uint64_t));
    }
    return TQ_OK;
  }
  // (the scoring pass reads term records: saturated tfs, the block search; a phrase atom: positions)
  if (!b.cut.wgs.empty() || scored || !b.tqs.empty() || !b.slop_qs.empty()) {
    rc = sync_terms(s, s->stream);
    if (rc != TQ_OK) return rc;
  }
  rc = size_and_upload(b);
  if (rc != TQ_OK) return rc;
  s->last_batch_queries = n_queries;
  return call.device_out ? run_device(b) : run_host(b);
}

}  // namespace tqi
