// tq_all.cpp — AllQuery clauses (tq_query.terms[i] == TQ_TERM_ALL): the ONE restatement of what
// BooleanWeight::complex_scorer (boolean_weight.rs:114-171, 236-431, 440-456) makes of a flat query that holds them.
// remove_and_count_all_and_empty_scorers takes the bare AllScorers (boost exactly 1.0) and the EmptyScorers (absent
// terms) out of every occur's list and counts them; what is left decides the query:
//   1. a MustNot-All                                  -> EMPTY (:264-267)
//   2. m' = max(0, m - Should-Alls); m' > |S|          -> EMPTY (:269-279)
//   3. m' >= 2 and m' == |S|                           -> the Should clauses are Must clauses (:292-297)
//   4. nothing left, or only MustNot clauses           -> EMPTY (effective_must_scorer None -> EmptyScorer, :340-349)
//   5. Must lists                                      -> PLAIN: the Alls vanish, scores included (intersect_scorers
//                                                         over the lists alone, :132-134)
//   6. no Must list: ALL-BASED when an AllScorer comes back — effective_must_scorer's (:124-128: a Must-All, or in the
//      Ignored branch any All) or effective_should_scorer_for_union's (:152-163: a Should-All under minimum 0);
//      else PLAIN (the Should scorer alone, :398-401)
//   7. ALL-BASED: every doc (m' == 0) or the docs with at least m' Should clauses, minus the MustNot lists; score =
//      the Should sum + 1.0 — RequiredOptionalScorer(All, should), Intersection(All, should) and the union's SumCombiner
//      all add ONE AllScorer's 1.0 to the Should sum, however many All clauses there were.
// A boosted All is a BoostScorer: it is not removed and stays an always-present scorer, which changes no doc set (so
// counts and doc sets treat every All alike) but does change the order of the score sums: the scoring entry points
// take it only as the sole non-MustNot clause that holds anything (base = the boost).
// Pure host code: needs nothing from the segment.  parse_flat_clauses (counts, doc sets) and the top-k planner
// (tq_search.cpp) both start from all_query_form / all_strip_view.
#include "tq_internal.hpp"

#include <limits>

namespace tqi {

int all_query_form(const tq_query &q, AllForm &f, const char **why) {
  f = AllForm{};
  *why = "";
  if (!q.terms || q.n_terms == 0 || q.n_terms > TQ_MAX_TERMS) return *why = "n_terms out of range (1..TQ_MAX_TERMS) or no terms", TQ_ERR_INVALID;
  if (q.mode > TQ_MODE_BOOL) return *why = "unknown mode", TQ_ERR_INVALID;
  if (q.mode == TQ_MODE_BOOL && !q.occurs) return *why = "TQ_MODE_BOOL without occurs", TQ_ERR_INVALID;
  const bool has_all = query_has_all(q);
  if (has_all && q.mode == TQ_MODE_PHRASE) return *why = "a match-all clause inside a phrase", TQ_ERR_INVALID;
  if (has_all && bool_query_is_tree(q)) return *why = "a match-all clause inside a nested boolean query", TQ_ERR_UNSUPPORTED;
  // the clauses: an All is one of its own; lists that share a clause_of value are one clause (a union)
  struct Clause {
    uint32_t id, occur;
    bool has_list = false, all = false;
  };
  Clause cl[TQ_MAX_TERMS];
  uint32_t n_cl = 0, n_boosted = 0;
  float boost = 1.0f;
  for (uint32_t i = 0; i < q.n_terms; ++i) {
    uint32_t occur = q.mode == TQ_MODE_AND ? (uint32_t)TQ_MUST : (uint32_t)TQ_SHOULD, id = i;
    if (q.mode == TQ_MODE_BOOL) {
      occur = q.occurs[i];
      if (occur > TQ_MUST_NOT) return *why = "occur out of range", TQ_ERR_INVALID;
      if (q.clause_of) id = q.clause_of[i];
    }
    const bool all = q.terms[i] == TQ_TERM_ALL;
    uint32_t c = 0;
    while (c < n_cl && cl[c].id != id) ++c;
    if (c < n_cl && (all || cl[c].all)) return *why = "a match-all clause inside a union (it shares a clause_of value)", TQ_ERR_UNSUPPORTED;
    if (c == n_cl) {
      cl[n_cl].id = id;
      cl[n_cl].occur = occur;
      ++n_cl;
    }
    if (all) {
      cl[c].all = true;
      if (q.weights && !std::isfinite(q.weights[i])) return *why = "the boost of a match-all clause is not finite", TQ_ERR_INVALID;
      if (q.weights && q.weights[i] != 1.0f && occur != TQ_MUST_NOT) {
        ++n_boosted;
        boost = q.weights[i];
      }
    } else if (q.terms[i] != TQ_TERM_ABSENT) {
      cl[c].has_list = true;
      f.keep_mask |= 1u << i;
    }
  }
  uint32_t a_must = 0, a_should = 0, a_not = 0, n_must = 0, n_should = 0;
  bool absent_must = false;
  for (uint32_t c = 0; c < n_cl; ++c) {
    const Clause &C = cl[c];
    if (C.all)
      ++(C.occur == TQ_MUST ? a_must : C.occur == TQ_SHOULD ? a_should : a_not);
    else if (!C.has_list)
      absent_must = absent_must || C.occur == TQ_MUST;  // an EmptyScorer among the Must scorers (:250-252)
    else if (C.occur != TQ_MUST_NOT)
      ++(C.occur == TQ_MUST ? n_must : n_should);
  }
  const uint32_t m = q.mode == TQ_MODE_BOOL ? q.min_should_match : 0u;
  const uint32_t m1 = m > a_should ? m - a_should : 0u;
  f.min_should = m1;
  const bool should_is_must = m1 >= 2 && m1 == n_should;
  bool empty = absent_must || a_not > 0 || m1 > n_should;
  empty = empty || (n_must == 0 && n_should == 0 && a_must == 0 && a_should == 0);
  if (empty) {
    f.kind = TQ_ALL_EMPTY;
    f.min_should = f.keep_mask = 0;
    return TQ_OK;
  }
  if (n_must > 0 || should_is_must) {
    f.kind = TQ_ALL_PLAIN;
  } else if (a_must > 0 || (a_should > 0 && m1 == 0)) {
    f.kind = TQ_ALL_BASED;
    f.base = 1.0f;
  } else {
    f.kind = TQ_ALL_PLAIN;
  }
  // a BoostScorer(AllScorer) is an ordinary scorer: alone it is the query; beside others the sums take an order of their own
  if (n_boosted) {
    if (n_boosted == 1 && a_must + a_should == 1 && n_must + n_should == 0) {
      f.base = boost;
    } else {
      f.boost_mixed = true;
      f.base = std::numeric_limits<float>::quiet_NaN();
    }
  }
  return TQ_OK;
}

void all_strip_view(const tq_query &q, const AllForm &f, AllView &v) {
  v.q = q;
  v.q.nested_occurs = nullptr;  // (flat: all_query_form refused the trees)
  v.q.clause_min_should = nullptr;
  v.q.atom_of = nullptr;
  v.q.phrase_offsets = nullptr;
  uint32_t n = 0;
  for (uint32_t i = 0; i < q.n_terms; ++i) {
    if (!((f.keep_mask >> i) & 1u)) continue;
    v.pos[n] = i;
    v.terms[n] = q.terms[i];
    v.weights[n] = q.weights ? q.weights[i] : 1.0f;
    v.occurs[n] = q.occurs ? q.occurs[i] : 0;
    v.clause_of[n] = q.clause_of ? q.clause_of[i] : (uint8_t)i;
    ++n;
  }
  if (n == 0) {  // (EMPTY: an intersection with an absent list)
    v.terms[0] = TQ_TERM_ABSENT;
    v.weights[0] = 1.0f;
    v.occurs[0] = TQ_MUST;
    v.clause_of[0] = 0;
    v.pos[0] = 0;
    v.q.mode = TQ_MODE_AND;
    n = 1;
  }
  v.q.n_terms = n;
  v.q.terms = v.terms;
  v.q.weights = q.weights ? v.weights : nullptr;
  v.q.occurs = v.q.mode == TQ_MODE_BOOL ? v.occurs : nullptr;
  v.q.clause_of = v.q.mode == TQ_MODE_BOOL && q.clause_of ? v.clause_of : nullptr;
  v.q.min_should_match = f.min_should;
}

}  // namespace tqi

extern "C" int tq_all_query_form(const tq_query *q, tq_all_form *out) {
  using namespace tqi;
  if (!q || !out) return fail(TQ_ERR_INVALID, "tq_all_query_form: null argument");
  AllForm f;
  const char *why = "";
  const int rc = all_query_form(*q, f, &why);
  out->kind = f.kind;
  out->base = f.base;
  out->min_should = f.min_should;
  out->keep_mask = f.keep_mask;
  if (rc != TQ_OK) return fail(rc, "tq_all_query_form: %s", why);
  if (f.boost_mixed)
    return fail(TQ_ERR_UNSUPPORTED, "tq_all_query_form: a boosted match-all clause beside another scoring clause or a second match-all clause");
  return TQ_OK;
}
