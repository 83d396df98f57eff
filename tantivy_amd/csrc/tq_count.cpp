// tq_count_batch: the Count collector (src/collector/count_collector.rs:39-80).  Queries whose lists all
// have a bitmap and whose doc set is cheaper to get from bitmap words than from postings are counted by
// tq_count.hip (a bitwise expression per 32 docs); the others by an exhaustive scan with the smallest top-k.
#include "tq_internal.hpp"

#include <deque>
#include <unordered_map>

namespace tqi {

// The clauses of a flat query (AND, OR, or TQ_MODE_BOOL over terms and unions of terms): what count_expression and
// docset_expression (tq_docset.cpp) both start from.  FLAT_UNSUPPORTED: a phrase or a nested query; FLAT_INVALID:
// malformed input (*why says what).
int parse_flat_clauses(tq_segment *s, const tq_query &q, FlatClauses &fc, const char **why) {
  fc.n_cl = fc.n_must = fc.n_should = 0;
  fc.empty = fc.all_based = fc.all_boost_mixed = false;
  fc.msm = 0;
  *why = "";
  if (query_has_all(q)) {  // AllQuery clauses: the clauses of what is left of the query (tq_all.cpp)
    AllForm f;
    const int arc = all_query_form(q, f, why);
    if (arc != TQ_OK) return arc == TQ_ERR_UNSUPPORTED ? FLAT_UNSUPPORTED : FLAT_INVALID;
    AllView v;
    all_strip_view(q, f, v);
    const int prc = parse_flat_clauses(s, v.q, fc, why);
    if (prc != FLAT_OK) return prc;
    for (uint32_t c = 0; c < fc.n_cl; ++c)
      for (uint32_t i = 0; i < fc.cl[c].n; ++i) fc.cl[c].pos[i] = v.pos[fc.cl[c].pos[i]];
    fc.all_based = f.kind == TQ_ALL_BASED;
    fc.all_base = f.base;
    fc.all_boost_mixed = f.boost_mixed;
    return FLAT_OK;
  }
  fc.msm = q.mode == TQ_MODE_BOOL ? q.min_should_match : 0u;
  if (!q.terms || q.n_terms == 0 || q.n_terms > TQ_MAX_TERMS) return *why = "n_terms out of range (1..TQ_MAX_TERMS) or no terms", FLAT_INVALID;
  if (q.mode == TQ_MODE_PHRASE) return *why = "a phrase query", FLAT_UNSUPPORTED;
  if (q.mode > TQ_MODE_BOOL) return *why = "unknown mode", FLAT_INVALID;
  if (q.mode == TQ_MODE_BOOL && !q.occurs) return *why = "TQ_MODE_BOOL without occurs", FLAT_INVALID;
  if (bool_query_is_tree(q)) return *why = "a nested boolean query", FLAT_UNSUPPORTED;
  FlatClauses::Clause *cl = fc.cl;
  uint32_t n_cl = 0;
  for (uint32_t i = 0; i < q.n_terms; ++i) {
    uint32_t occur = q.mode == TQ_MODE_AND ? TQ_MUST : TQ_SHOULD;
    uint32_t id = i;
    if (q.mode == TQ_MODE_BOOL) {
      occur = q.occurs[i];
      if (occur > TQ_MUST_NOT) return *why = "occur out of range", FLAT_INVALID;
      if (q.clause_of) id = q.clause_of[i];
    }
    uint32_t c = 0;
    while (c < n_cl && cl[c].id != id) ++c;
    if (c == n_cl) {
      cl[n_cl] = FlatClauses::Clause{};
      cl[n_cl].id = id;
      cl[n_cl].occur = occur;
      ++n_cl;
    } else if (cl[c].occur != occur) {
      return *why = "mixed occurs in one clause", FLAT_INVALID;
    }
    const uint32_t h = q.terms[i];
    if (h == TQ_TERM_ABSENT) continue;
    if (h >= s->terms.size()) return *why = "term handle out of range", FLAT_INVALID;
    cl[c].pos[cl[c].n] = i;
    cl[c].terms[cl[c].n++] = h;
    cl[c].cost += s->terms[h].doc_freq;
  }
  fc.n_cl = n_cl;
  // BooleanWeight::complex_scorer (boolean_weight.rs:236-431), as plan_bool_query restates it
  for (uint32_t c = 0; c < n_cl; ++c) {
    if (cl[c].occur == TQ_MUST) {
      if (cl[c].n == 0) fc.empty = true;
      ++fc.n_must;
    } else if (cl[c].n) {
      if (cl[c].occur == TQ_SHOULD) ++fc.n_should;
    }
  }
  return FLAT_OK;
}

// The query as a bitwise expression, or false if it has to be scanned (a phrase, a list without a bitmap,
// minimum_number_should_match >= 2 over fewer Should clauses than that, malformed input — the scan reports it).
// `known` = the count is known without looking (an absent Must term, MustNot clauses only, ...): 0 matches.
bool count_expression(tq_segment *s, const tq_query &q, TqkCountQuery &cq, bool &known, uint64_t &driver_postings,
                      std::unordered_map<uint32_t, uint32_t> &temp_slot, uint32_t max_temp) {
  known = false;
  driver_postings = 0;
  cq = TqkCountQuery{};
  FlatClauses fc;
  const char *why;
  if (parse_flat_clauses(s, q, fc, &why) != FLAT_OK) return false;
  using Clause = FlatClauses::Clause;
  const Clause *cl = fc.cl;
  const uint32_t n_cl = fc.n_cl, n_must = fc.n_must, n_should = fc.n_should;
  bool empty = fc.empty;
  // a list without a bitmap gets one for the duration of the batch (count_scatter_kernel), while the
  // batch's scratch has room for another
  for (uint32_t c = 0; c < n_cl; ++c)
    for (uint32_t i = 0; i < cl[c].n; ++i) {
      const uint32_t h = cl[c].terms[i];
      if (!expression_bitmap(s, s->terms[h]) && !temp_slot.count(h) && temp_slot.size() >= max_temp) return false;
    }
  if (fc.all_based) return false;  // (count_batch counts these itself: never the scan)
  uint32_t msm = fc.msm;
  if (msm > n_should) empty = true;
  bool should_is_must = false;
  if (!empty && msm >= 2) {
    if (msm != n_should) return false;  // "at least m of n": not a bitwise expression of this shape
    should_is_must = true;              // all of them: Must clauses
    msm = 0;
  }
  if (n_must == 0 && n_should == 0) empty = true;
  if (empty) {
    known = true;
    return true;
  }
  uint32_t n = 0;
  uint64_t must_cost = ~0ull, should_cost = 0;
  auto put = [&](const Clause &c, uint32_t kind, bool clause_union) {
    for (uint32_t i = 0; i < c.n; ++i) {
      const TermHost &th = s->terms[c.terms[i]];
      if (expression_bitmap(s, th)) {
        cq.dense[n] = (const uint2 *)th.dense_blob;
      } else {  // (the slot for now; the pointer once the scratch is allocated)
        const uint32_t slot = temp_slot.emplace(c.terms[i], (uint32_t)temp_slot.size()).first->second;
        cq.dense[n] = (const uint2 *)(uintptr_t)slot;
        cq.narrow |= 1u << n;
      }
      cq.kinds |= kind << (2u * n);
      if (kind == TQK_COUNT_MUST && (!clause_union || i + 1 == c.n)) cq.clause_end |= 1u << n;
      ++n;
    }
  };
  const bool has_must = n_must > 0 || should_is_must;
  for (uint32_t c = 0; c < n_cl; ++c) {
    if (cl[c].occur == TQ_MUST || (should_is_must && cl[c].occur == TQ_SHOULD && cl[c].n)) {
      put(cl[c], TQK_COUNT_MUST, true);
      must_cost = std::min(must_cost, cl[c].cost);
    }
  }
  for (uint32_t c = 0; c < n_cl; ++c)
    if (cl[c].occur == TQ_MUST_NOT && cl[c].n) put(cl[c], TQK_COUNT_NOT, false);
  if (!should_is_must)
    for (uint32_t c = 0; c < n_cl; ++c)
      if (cl[c].occur == TQ_SHOULD && cl[c].n) {
        // with Must clauses and no minimum the Should lists do not change the doc set
        if (has_must && msm == 0) continue;
        put(cl[c], TQK_COUNT_SHOULD, false);
        should_cost += cl[c].cost;
      }
  cq.n_terms = n;
  cq.flags = (has_must ? TQK_COUNT_HAS_MUST : 0u) | ((has_must && msm == 1) ? TQK_COUNT_NEED_SHOULD : 0u);
  driver_postings = has_must ? must_cost : should_cost;  // what a scan would walk: the cheapest Must clause / the union
  return true;
}

int count_batch(tq_segment *s, const tq_query *queries, uint32_t n_queries, uint32_t *out_counts) {
  // A bitmap word costs 8 bytes per list per 32 docs whatever the lists hold; a scan decodes the
  // postings of the driving clause (and probes the others): bitmaps when the driving clause holds at
  // least max_doc / ratio postings per list of the expression ("count_bitmap_ratio", 0 = never).
  static const uint32_t kRatioEnv = tune_u32("TQ_COUNT_BITMAP_RATIO", 0xFFFFFFFFu);
  const uint32_t kRatio = kRatioEnv != 0xFFFFFFFFu ? kRatioEnv : (uint32_t)s->opt.count_bitmap_ratio;
  static const uint64_t kTempBudget = (uint64_t)std::max<uint32_t>(1u, tune_u32("TQ_COUNT_TEMP_MB", 1024)) << 20;
  const uint32_t n_words = (uint32_t)(((uint64_t)s->max_doc + 31u) / 32u);
  const uint32_t words_per_list = (n_words + 63u) & ~63u;
  const uint32_t max_temp = (uint32_t)std::min<uint64_t>(4096u, kTempBudget / ((uint64_t)words_per_list * 4u));
  std::vector<TqkCountQuery> cqs;
  std::vector<uint32_t> bitmap_q, scan_q, all_q;
  std::unordered_map<uint32_t, uint32_t> temp_slot, trial;  // lists without a bitmap -> slot of the batch's scratch
  // Queries with AllQuery clauses (tq_all.cpp): EMPTY counts 0; PLAIN is counted as its stripped view is; ALL-BASED
  // never falls back to the scan — without a MustNot list and a minimum it counts the segment's alive docs, no kernel
  // at all; the others go through the doc-set count pass (its expression masks the segment's last word).
  std::deque<AllView> views;
  std::vector<tq_query> eff;
  std::vector<uint8_t> done;
  const tq_query *const given = queries;
  s->last_batch_slop = false;  // (set again by the doc-set pass, the last one of this call, if it holds a sloppy phrase)
  for (uint32_t qi = 0; qi < n_queries; ++qi) {
    if (!query_has_all(given[qi])) continue;
    if (eff.empty()) {
      eff.assign(given, given + n_queries);
      done.assign(n_queries, 0);
    }
    AllForm f;
    const char *why = "";
    const int arc = all_query_form(given[qi], f, &why);
    if (arc != TQ_OK) return fail(arc, "tq_count_batch: query %u: %s", qi, why);
    views.emplace_back();
    all_strip_view(given[qi], f, views.back());
    eff[qi] = views.back().q;
    if (f.kind != TQ_ALL_BASED) continue;
    done[qi] = 1;
    bool any_not = false;
    for (uint32_t i = 0; i < given[qi].n_terms; ++i) {
      if (!((f.keep_mask >> i) & 1u)) continue;
      if (given[qi].terms[i] >= s->terms.size()) return fail(TQ_ERR_INVALID, "tq_count_batch: query %u: term handle out of range", qi);
      any_not = any_not || (given[qi].occurs && given[qi].occurs[i] == TQ_MUST_NOT);
    }
    if (f.min_should == 0 && !any_not)
      out_counts[qi] = s->d_alive ? s->alive_docs : s->max_doc;
    else
      all_q.push_back(qi);
  }
  if (!eff.empty()) queries = eff.data();
  // Sloppy phrases (TQ_MODE_PHRASE with slop > 0, tq_phrase_slop.cpp): Count runs the reference's NON-SCORING PhraseScorer,
  // whose verdict differs from the scoring one — never the scan; the doc-set count pass over their match bits.
  for (uint32_t qi = 0; qi < n_queries; ++qi) {
    if (!given[qi].slop) continue;
    SlopView sv;
    const int vrc = slop_view(s, given[qi], qi, "tq_count_batch", sv, false);  // (refusals under the caller's index)
    if (vrc != TQ_OK) return vrc;
    if (done.empty()) done.assign(n_queries, 0);
    done[qi] = 1;
    all_q.push_back(qi);
  }
  // Queries that name a term set (tq_termset.cpp) are never scanned — a set has no postings to walk: the bitmap kernel
  // whatever "count_bitmap_ratio" says, or — "at least m of n" — the doc-set count pass.
  std::vector<uint8_t> set_q;
  for (uint32_t qi = 0; s->n_set_slots && qi < n_queries; ++qi) {
    bool has = false;
    const int src = check_set_query(s, given[qi], qi, "tq_count_batch", &has);
    if (src != TQ_OK) return src;
    if (has && set_q.empty()) set_q.assign(n_queries, 0);
    if (has) set_q[qi] = 1;
  }
  // Multi-field segments (tq_fields.cpp): a phrase over terms of different fields is refused here, under the caller's
  // index (the scan below sees a sub-batch); looked for only while the segment holds a term of a field != 0.
  for (uint32_t qi = 0; s->n_field_terms && qi < n_queries; ++qi)
    if (query_names_field(s, given[qi])) {
      const int frc = check_field_query(s, given[qi], qi, "tq_count_batch");
      if (frc != TQ_OK) return frc;
    }
  for (uint32_t qi = 0; qi < n_queries; ++qi) {
    if (!done.empty() && done[qi]) continue;
    TqkCountQuery cq;
    bool known = false;
    uint64_t driver = 0;
    trial = temp_slot;  // (a query that ends up scanned leaves no slots behind)
    const bool names_set = !set_q.empty() && set_q[qi];
    const bool expr = (kRatio || names_set) && count_expression(s, queries[qi], cq, known, driver, trial, max_temp);
    if (expr && known) {
      out_counts[qi] = 0;
    } else if (expr && (names_set || driver * kRatio >= (uint64_t)cq.n_terms * s->max_doc)) {
      cqs.push_back(cq);
      bitmap_q.push_back(qi);
      temp_slot.swap(trial);
    } else if (names_set) {
      // (what the doc-set pass would refuse is reported here, under the caller's index: that pass sees a sub-batch)
      TqkDocsetQuery dq;
      const char *why = "";
      const int drc = docset_expression(s, given[qi], dq, &why);
      if (drc != FLAT_OK) return fail(drc == FLAT_UNSUPPORTED ? TQ_ERR_UNSUPPORTED : TQ_ERR_INVALID, "tq_count_batch: query %u: %s", qi, why);
      all_q.push_back(qi);
    } else {
      scan_q.push_back(qi);
    }
  }
  HIP_TRY(hipSetDevice(s->device));
  uint32_t mask = 0;
  uint64_t algo_bytes = 0;
  if (!scan_q.empty()) {
    // every match has to be visited: exhaustive scan, smallest top-k
    const uint32_t n = (uint32_t)scan_q.size();
    std::vector<tq_query> qs(n);
    for (uint32_t i = 0; i < n; ++i) {
      qs[i] = queries[scan_q[i]];
      qs[i].k = 1;
    }
    std::vector<float> sc(n);
    std::vector<uint32_t> dc(n), ct(n), mc(n);
    CallOpts co;
    int rc = resolve_opts(s, nullptr, co);
    if (rc != TQ_OK) return rc;
    co.exhaustive = true;  // per call: the segment's options are not touched
    rc = search_batch_host(s, qs.data(), n, 1, sc.data(), dc.data(), ct.data(), co);
    if (rc != TQ_OK) return rc;
    rc = tq_last_batch_match_counts(s, mc.data(), n);
    if (rc != TQ_OK) return rc;
    for (uint32_t i = 0; i < n; ++i) out_counts[scan_q[i]] = mc[i];
    mask = s->stats.kernel_mask;
    algo_bytes = s->stats.algorithmic_bytes;
  } else {
    const int wrc = wait_segment_idle(s);
    if (wrc != TQ_OK) return wrc;
  }
  if (!bitmap_q.empty()) {
    const uint32_t n = (uint32_t)bitmap_q.size();
    int rc = s->d_count_queries.ensure((size_t)n * sizeof(TqkCountQuery));
    if (rc == TQ_OK) rc = s->d_count_out.ensure((size_t)n * sizeof(uint32_t));
    if (rc != TQ_OK) return rc;
    if (!temp_slot.empty()) {  // the batch's lists without a bitmap, as bits
      const int src = sync_terms(s, s->stream);
      if (src != TQ_OK) return src;
      std::vector<uint4> wgs;
      for (const auto &kv : temp_slot) push_scatter_work(wgs, s, kv.first, kv.second);
      rc = s->d_count_bits.ensure((size_t)temp_slot.size() * words_per_list * sizeof(uint32_t));
      if (rc == TQ_OK) rc = s->d_count_wgs.ensure(wgs.size() * sizeof(uint4));
      if (rc != TQ_OK) return rc;
      HIP_TRY(hipMemsetAsync(s->d_count_bits.p, 0, (size_t)temp_slot.size() * words_per_list * sizeof(uint32_t), s->stream));
      HIP_TRY(hipMemcpyAsync(s->d_count_wgs.p, wgs.data(), wgs.size() * sizeof(uint4), hipMemcpyHostToDevice, s->stream));
      const hipError_t se = tqk_launch_count_scatter(s->dseg, s->d_terms, (const uint4 *)s->d_count_wgs.p, (uint32_t)wgs.size(),
                                                     (uint32_t *)s->d_count_bits.p, words_per_list, s->stream);
      if (se != hipSuccess) return fail(TQ_ERR_HIP, "count scatter launch: %s", hipGetErrorString(se));
      for (TqkCountQuery &cq : cqs)
        for (uint32_t m = 0; m < cq.n_terms; ++m)
          if ((cq.narrow >> m) & 1u)
            cq.dense[m] = (const uint2 *)((const uint32_t *)s->d_count_bits.p + (size_t)(uintptr_t)cq.dense[m] * words_per_list);
    }
    HIP_TRY(hipMemcpyAsync(s->d_count_queries.p, cqs.data(), (size_t)n * sizeof(TqkCountQuery), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemsetAsync(s->d_count_out.p, 0, (size_t)n * sizeof(uint32_t), s->stream));
    TqkCountParams p{};
    p.queries = (const TqkCountQuery *)s->d_count_queries.p;
    p.alive = s->d_alive;
    p.out_counts = (uint32_t *)s->d_count_out.p;
    p.n_queries = n;
    p.n_words = n_words;
    const hipError_t e = tqk_launch_count_bitmaps(p, s->stream);
    if (e != hipSuccess) return fail(TQ_ERR_HIP, "count kernel launch: %s", hipGetErrorString(e));
    std::vector<uint32_t> got(n);
    HIP_TRY(hipMemcpyAsync(got.data(), s->d_count_out.p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    for (uint32_t i = 0; i < n; ++i) {
      out_counts[bitmap_q[i]] = got[i];
      algo_bytes += (uint64_t)cqs[i].n_terms * p.n_words * 4u;  // the lists' bits (the rank halves of the words ride along)
    }
    mask |= TQ_KERNEL_COUNT_BITMAPS;
  }
  if (!all_q.empty()) {  // ALL-BASED queries with a MustNot list or a minimum: the doc-set count pass, no doc written
    const uint32_t n = (uint32_t)all_q.size();
    std::vector<tq_query> qs(n);
    for (uint32_t i = 0; i < n; ++i) qs[i] = given[all_q[i]];
    std::vector<uint64_t> starts((size_t)n + 1u);
    // (sloppy phrases are named, and their overflow words indexed, by the caller's query: all_q)
    DocsetCall call("tq_count_batch", DocsetConsumer::kCount);
    call.out_starts = starts.data();
    call.caller_q = all_q.data();
    call.n_caller = n_queries;
    const int rc = docset_batch(s, qs.data(), n, call);
    // a carried list over the cap (the verdict comes behind the count pass: `starts` is filled): the counts of the other
    // queries are written and valid, the words of this batch stay readable (tq_last_batch_slop_overflows)
    // (last_batch_slop is set once every query is checked and planned: the one refusal behind that is the overflow verdict)
    const bool overflowed = rc == TQ_ERR_UNSUPPORTED && s->last_batch_slop;
    for (uint32_t i = 0; (rc == TQ_OK || overflowed) && i < n; ++i) out_counts[all_q[i]] = (uint32_t)(starts[i + 1u] - starts[i]);
    s->slop_over_words = n_queries;
    if (rc != TQ_OK) return rc;
    algo_bytes += s->stats.algorithmic_bytes;
    mask |= TQ_KERNEL_DOCSET | (s->stats.kernel_mask & (TQ_KERNEL_PHRASE_SLOP | TQ_KERNEL_DOCSET_TREE));
  }
  s->stats.kernel_mask = mask;
  s->stats.algorithmic_bytes = algo_bytes;
  s->slop_over_words = n_queries;  // (the sub-batches above counted their own queries)
  return TQ_OK;
}

}  // namespace tqi
