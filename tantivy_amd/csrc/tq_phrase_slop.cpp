// tq_phrase_slop.cpp — the planner side of TQ_MODE_PHRASE with slop > 0 (kernels: tq_phrase_slop.hip; the contract:
// tantivy_amd.h "Sloppy phrases"): validation, the query as a one-atom tree in COST order, its
// descriptor, and the overflow verdict.  The routes that use it: tq_search.cpp (a launch group of its own, kGSlop),
// tq_docset.cpp (match bits under "docset_trees"), tq_count.cpp (through the doc-set route's count pass).
// Part of the C ABI library of include/tantivy_amd.h (internal declarations: tq_internal.hpp).
#include "tq_internal.hpp"

namespace tqi {

static_assert(TQK_SLOP_CARRY_CAP == TQ_SLOP_CARRY_CAP, "the kernels' cap is the header's");
static_assert(TQ_SLOP_CARRY_CAP >= 32u, "the contract promises at least 32 entries");
static_assert(TQK_SLOP_MAX_TERMS == 8u, "device phrases take 2..8 terms");

int slop_view(const tq_segment *s, const tq_query &q, uint32_t qi, const char *fn, SlopView &out, bool scored) {
  if (q.mode != TQ_MODE_PHRASE)
    return fail(TQ_ERR_INVALID, "%s: query %u: slop %u outside TQ_MODE_PHRASE (only a PhraseQuery has a slop)", fn, qi, q.slop);
  if (q.slop > TQ_MAX_SLOP)
    return fail(TQ_ERR_UNSUPPORTED, "%s: query %u: slop %u above TQ_MAX_SLOP (%u)", fn, qi, q.slop, TQ_MAX_SLOP);
  if (q.n_terms < 2 || q.n_terms > TQ_MAX_TERMS || !q.terms || !q.phrase_offsets)
    return fail(TQ_ERR_INVALID, "%s: query %u: a phrase needs >= 2 terms and offsets", fn, qi);
  if (q.n_terms > TQK_SLOP_MAX_TERMS)
    return fail(TQ_ERR_UNSUPPORTED, "%s: query %u: device phrases take at most %u terms", fn, qi, TQK_SLOP_MAX_TERMS);
  if (scored && (!q.weights || !std::isfinite(q.weights[0])))
    return fail(TQ_ERR_INVALID, "%s: query %u: a phrase needs a finite weight in weights[0]", fn, qi);
  for (uint32_t i = 0; i < q.n_terms; ++i) {
    const uint32_t h = q.terms[i];
    if (h == TQ_TERM_ABSENT) continue;
    if (h == TQ_TERM_ALL) return fail(TQ_ERR_INVALID, "%s: query %u: a match-all clause inside a phrase", fn, qi);
    if (h >= s->terms.size()) return fail(TQ_ERR_INVALID, "%s: query %u: unknown term handle %u", fn, qi, h);
    if (is_term_set(s, h)) return fail(TQ_ERR_INVALID, "%s: query %u: a term set inside a phrase", fn, qi);
    if (term_field_of(s, h))
      return fail(TQ_ERR_UNSUPPORTED, "%s: query %u: a sloppy phrase over terms of field %u stays on the CPU (field 0 only)", fn, qi, term_field_of(s, h));
  }
  // Intersection::new: docsets.sort_by_key(cost), stable; the cost of a posting list is its doc freq
  uint32_t order[TQ_MAX_TERMS];
  for (uint32_t i = 0; i < q.n_terms; ++i) order[i] = i;
  auto df = [&](uint32_t i) { return q.terms[i] == TQ_TERM_ABSENT ? 0u : s->terms[q.terms[i]].doc_freq; };
  std::stable_sort(order, order + q.n_terms, [&](uint32_t x, uint32_t y) { return df(x) < df(y); });
  tq_query ordered = q;
  for (uint32_t i = 0; i < q.n_terms; ++i) {
    out.terms[i] = q.terms[order[i]];
    out.offsets[i] = q.phrase_offsets[order[i]];
  }
  ordered.terms = out.terms;
  ordered.phrase_offsets = out.offsets;
  ordered.slop = 0;  // (the view is a TQ_MODE_BOOL query: the slop travels beside it)
  docset_tree_view(ordered, out.v, scored);
  return TQ_OK;
}

int plan_slop_query(tq_segment *s, const tq_query &view, uint32_t qi, uint32_t slop, TqdSlopQuery &sq, uint64_t &qbytes, bool result_bitmap) {
  TqdTreeQuery tq;
  uint64_t list_bytes = 0;  // (the tree planner's figure counts the packed lists: not what this route reads)
  const int rc = plan_tree_query(s, view, qi, tq, list_bytes, s->share_table_lo);
  if (rc != TQ_OK) return rc;
  sq = TqdSlopQuery{};
  sq.k = view.k;
  sq.slop = slop;
  sq.out_q = qi;
  if (tq.n_terms == 0) return TQ_OK;  // an absent term: Ok(None) -> EmptyScorer (phrase_weight.rs)
  if (tq.n_clauses != 1 || tq.n_terms < 2 || tq.n_terms > TQK_SLOP_MAX_TERMS)
    return fail(TQ_ERR_INVALID, "query %u: a sloppy phrase came out of the tree planner as %u clauses of %u terms", qi, tq.n_clauses, tq.n_terms);
  sq.n_terms = tq.n_terms;
  sq.weight_bits = tq.weight_bits[0];
  for (uint32_t t = 0; t < tq.n_terms; ++t) {
    sq.dense_off[t] = tq.dense_off[t];
    sq.tf8_off[t] = tq.tf8_off[t];
    sq.dir_off[t] = tq.dir_off[t];
    sq.phrase_off[t] = tq.phrase_off[t];
    sq.handle[t] = tq.handle[t];
  }
  const uint64_t n_words = (s->max_doc + 31u) / 32u;
  qbytes += (uint64_t)(tq.n_terms + (result_bitmap ? 2u : 1u)) * n_words * 4u;
  return TQ_OK;
}

int slop_overflow_fail(const char *fn, uint32_t qi, uint32_t docs) {
  return fail(TQ_ERR_UNSUPPORTED, "%s: query %u: carried position list over TQ_SLOP_CARRY_CAP (%u entries) in %u candidate doc%s: its rows are not valid, the query stays on the CPU",
              fn, qi, TQ_SLOP_CARRY_CAP, docs, docs == 1u ? "" : "s");
}

int slop_overflow_verdict(const char *fn, const uint32_t *over, uint32_t n_queries) {
  for (uint32_t qi = 0; qi < n_queries; ++qi)
    if (over[qi]) return slop_overflow_fail(fn, qi, over[qi]);
  return TQ_OK;
}

int slop_overflow_readback(tq_segment *s, const char *fn) {
  if (!s->last_batch_slop) return TQ_OK;
  std::vector<uint32_t> over(s->slop_over_words);
  HIP_TRY(hipMemcpy(over.data(), s->d_slop_over.p, over.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return slop_overflow_verdict(fn, over.data(), (uint32_t)over.size());
}

}  // namespace tqi

extern "C" int tq_last_batch_slop_overflows(tq_segment *s, uint32_t *out, uint32_t n) {
  using namespace tqi;
  if (!s || !out) return fail(TQ_ERR_INVALID, "tq_last_batch_slop_overflows: null argument");
  TQ_SEGMENT_LOCK(s);
  const uint32_t had = s->slop_over_words;  // (the CALLER's batch: tq_count_batch runs sub-batches of its own)
  if (n > had) return fail(TQ_ERR_INVALID, "the last batch had %u queries", had);
  if (!s->last_batch_slop) {
    memset(out, 0, (size_t)n * sizeof(uint32_t));
    return TQ_OK;
  }
  HIP_TRY(hipSetDevice(s->device));
  {
    const int wrc = wait_segment_idle(s);
    if (wrc != TQ_OK) return wrc;
  }
  HIP_TRY(hipMemcpy(out, s->d_slop_over.p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return TQ_OK;
}
