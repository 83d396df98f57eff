// tq_search.cpp — one batch of queries on one segment: validation, launch groups, the planners, the staging blob,
// kernel launches and merges (tq_search_batch, tq_search_batch_device and their _opts forms)
// Part of the C ABI library of include/tantivy_amd.h (internal declarations: tq_internal.hpp).
#include "tq_internal.hpp"

namespace tqi {
namespace {

using Clock = std::chrono::steady_clock;

// The switches more than one stage reads (read once, at the first batch).
struct Knobs {
  // boolean queries in the shared launch when their lists have a bitmap + tf bytes, or a range directory (TQ_BS_RDIR)
  bool use_bshare = tune_u32("TQ_BSHARE", 1) != 0, bs_rdir = tune_u32("TQ_BS_RDIR", 1) != 0;
  // the shared-intersection launch for AND queries whose leader leads >= ashare_min of them (round 4 asked for 4: two
  // kernel families sharing the chip cost more than lone leads do — 1 024 queries 1.39 -> 1.17 ms, mixed 7.6 -> 7.3)
  bool use_ashare = tune_u32("TQ_ASHARE", 1) != 0;
  uint32_t ashare_min = std::max<uint32_t>(1u, tune_u32("TQ_AS_MIN_LEADS", 1));
  // the shared-union launch (term-major, tq_ushare.hip) for pure unions, pruned, k <= 128, <= 8 terms, with a doc matrix
  bool use_ushare = tune_u32("TQ_USHARE", 1) != 0;
  uint32_t debug = tune_u32("TQ_DEBUG", 0);  // the kernels' ablation / work-counter bits (profiling only)
};
const Knobs &knobs() {
  static const Knobs k;
  return k;
}

// What one batch carries from stage to stage.
struct Batch {
  tq_segment *s;  // the call
  const tq_query *queries;
  uint32_t n_queries, out_stride;
  float *out_scores;  // the rows
  uint32_t *out_docs, *out_counts;
  void *hip_stream;
  CallOpts co;
  uint32_t *out_segment_ords;  // tq_search_batch_device_rows: the rows' column of segment ordinals, or null
  uint32_t segment_ord;
  bool replan = false;  // plan_batch: a shared launch is over its list budget, co now keeps that family off
  hipStream_t st = nullptr;
  bool exhaustive = false, or_windows = false;
  Clock::time_point t0, t_route, t_routed, t_laid, t_waited, t_filled;  // TQ_TRACE's phases, host_plan_ms
  size_t terms_from = 0, terms_to = 0;  // term records appended to the device table through the staging blob
  std::vector<const float *> caches;    // the Bm25Weight caches, in order of first use (PlanScratch::q_cache)
  uint32_t n_union_queries = 0, n_bool_queries = 0, n_sparse2 = 0;
  uint32_t n_all_queries = 0;  // ALL-BASED queries (TQ_TERM_ALL clauses that make every doc a candidate): counted by strip_all_clauses
  const uint8_t *set_q = nullptr;  // per query: it names a term set (tq_termset.cpp) and is routed to the tree group; null: no
                                   // query of the batch does (flagged and counted by strip_all_clauses)
  const uint32_t *slop_q = nullptr;  // per query: its slop (a sloppy phrase, replaced by its one-atom tree view in COST order:
                                     // tq_phrase_slop.cpp) or 0; null: no query of the batch has one
  bool and_probe = false, ashare_on = false, ashare_and = false;
  uint32_t and_tile_cap = TQD_AND_TILE, dense_min_queries = 1;
  uint64_t unique_bytes = 0, dense_ratio = 0;
  PlanScratch *ps = nullptr;
  Group *groups = nullptr;  // ps->groups
  RouteTotals t;
  int cus = 256;
  size_t part_off_bytes[kNGroups] = {}, partial_bytes = 0;  // the groups' partial / result lists in one buffer
  struct Copy { size_t off; const void *src; size_t bytes; };  // one table of the staging blob
  std::vector<Copy> copies;  // the staging blob's contents (lay_out_stage)
  size_t stage = 0, o_caches = 0, o_terms = 0;
  int bx = 0;                     // which of the two staging buffers
  const uint8_t *ds = nullptr;    // ... on the device
  DeviceScratch *sc = nullptr;
  int slot = 0;
  uint32_t grid[kNGroups] = {};  // persistent grid of a result-list group
  std::vector<uint32_t> lmat_fill;  // leaders whose doc-matrix words in posting order this batch (re)fills (fill_leader_mats)
};

}  // namespace

// The address span of the side tables the shared launches reach through 32-bit offsets (8-byte units from its lower
// end: 32 GB), taken again when tables were added.
void update_table_span(tq_segment *s) {
  if (s->share_span_terms == s->terms.size()) return;  // (terms are prepared rarely)
  uint64_t lo = ~0ull, hi = 0;
  for (const TermHost &th : s->terms)
    for (const void *ptr : {th.dense_blob, th.tf8_blob, th.probe_dense_blob, th.probe_tf8_blob, th.rmax_blob, th.posdir_blob, th.probe_posdir_blob, th.lnorm_blob, th.lmat_blob})
      if (ptr) {
        lo = std::min<uint64_t>(lo, (uint64_t)ptr);
        hi = std::max<uint64_t>(hi, (uint64_t)ptr);
      }
  if (lo == ~0ull) lo = hi = 8;
  {  // the range directories' chunks: inside the span when it still fits with them (else the lists do without)
    uint64_t lo2 = lo, hi2 = hi;
    for (const auto &ch : s->rdir_chunks) {
      lo2 = std::min<uint64_t>(lo2, (uint64_t)ch.first);
      hi2 = std::max<uint64_t>(hi2, (uint64_t)ch.first + ch.second);
    }
    s->rdir_span_ok = !s->rdir_chunks.empty() && hi2 - (lo2 - 8) < (8ull << 32);
    if (s->rdir_span_ok) {
      lo = lo2;
      hi = hi2;
    }
  }
  s->share_table_lo = (lo - 8) & ~255ull;  // (256-byte aligned: a range directory's offset keeps its low five bits free for the shift)
  s->share_span_ok = hi - s->share_table_lo < (8ull << 32);
  s->share_span_terms = s->terms.size();
}

namespace {

// The batch's stream, the terms prepared on the copy stream, and the term records this batch appends to the device table.
int sync_term_records(Batch &b) {
  HIP_TRY(hipSetDevice(b.s->device));
  b.st = b.hip_stream ? (hipStream_t)b.hip_stream : b.s->stream;
  prep_apply_lmax(b.s, false);
  if (b.s->prep_pending >= 0) {  // terms uploaded by tq_term_prepare_batch on the copy stream: this batch reads them
    if (b.st != b.s->stream) HIP_TRY(hipStreamWaitEvent(b.st, b.s->ev_prep[b.s->prep_pending], 0));
    b.s->prep_pending = -1;
  }
  // Terms prepared since the last batch: their records are APPENDED to the device table through this batch's
  // staging blob (a device-to-device copy on the batch's stream, enqueue_copy) — the batches in flight never read
  // beyond the records they were planned with, so nothing waits for them.  A grown table, or a changed record that a
  // batch in flight may read, takes the blocking road (sync_terms).
  if (b.s->d_terms_dirty) {
    const size_t n_terms_now = b.s->h_dterms.size();
    if (b.s->d_terms && n_terms_now <= b.s->d_terms_cap && b.s->d_terms_dirty_from >= b.s->d_terms_synced) {
      b.terms_from = std::min(b.s->d_terms_dirty_from, n_terms_now);
      b.terms_to = n_terms_now;
    } else {
      const int rc = sync_terms(b.s, b.st);
      if (rc != TQ_OK) return rc;
    }
  }
  update_table_span(b.s);
  return TQ_OK;
}

// ONE pass over the caller's queries for everything that only needs a look at them: which Bm25Weight cache each
// uses (pointer identity; a handful per batch), how many are unions (a one-list intersection runs as one), whether
// there are boolean queries at all, how many 2-term intersections probe a list without tables (six passes over
// 10 000 80-byte descriptors were 0.16 ms of the headline step's 0.9 ms of host time)
void look_at_queries(Batch &b) {
  if (!b.s->plan) b.s->plan = new PlanScratch();
  b.ps = b.s->plan;
  b.ps->q_cache.resize(b.n_queries);
  const size_t n_terms_known = b.s->terms.size();
  const float *last_tc = nullptr;
  uint32_t last_idx = 0;
  for (uint32_t qi = 0; qi < b.n_queries; ++qi) {
    const tq_query &q = b.queries[qi];
    const float *tc = q.tf_cache;
    uint32_t cache_idx = 0;
    if (tc == last_tc && tc) {
      cache_idx = last_idx;
    } else if (tc) {
      // (a multi-field segment: tf_cache is one row per field, and the rows go up together — cache_idx names row 0)
      const uint32_t rows = b.s->n_fields;
      for (; cache_idx < b.caches.size(); cache_idx += rows)
        if (b.caches[cache_idx] == tc) break;
      if (cache_idx == b.caches.size())
        for (uint32_t f = 0; f < rows; ++f) b.caches.push_back(tc + (size_t)f * 256u);
      last_tc = tc;
      last_idx = cache_idx;
    }
    b.ps->q_cache[qi] = cache_idx;
    b.n_union_queries += (q.mode == TQ_MODE_OR || (q.mode == TQ_MODE_AND && q.n_terms == 1)) ? 1u : 0u;
    b.n_bool_queries += q.mode == TQ_MODE_BOOL ? 1u : 0u;
    if (q.mode == TQ_MODE_AND && q.n_terms == 2 && q.terms && q.terms[0] < n_terms_known && q.terms[1] < n_terms_known) {
      const TermHost &ta = b.s->terms[q.terms[0]], &tb = b.s->terms[q.terms[1]];
      const TermHost &probed = tb.doc_freq < ta.doc_freq ? ta : tb;
      if (!(probed.dense_blob && probed.tf8_blob) && !(probed.rdir_blob && b.s->rdir_span_ok)) ++b.n_sparse2;
    }
  }
}

// Probe tables for the lists that boolean queries and (and_probe) 2-term intersections would probe without a bitmap.
int build_flat_probe_tables(Batch &b) {
  // 2-term intersections that probe a list without tables of its own: on the per-query kernel they run on
  // the side stream next to the shared launch, almost for free while they are few (5 % of the headline
  // batch: pulling them into the shared launch cost 7 % of kernel time — no doc-matrix column, so nothing
  // filters their docs before the scoring stage — for the same step time); when they are many (22 % at
  // 4 096 terms) the shared launch with probe tables is 12 % faster.  TQ_AS_PROBE: 0 never, 1 from 10 % of
  // the batch (default), 2 always.
  static const uint32_t kProbeAnd = tune_u32("TQ_AS_PROBE", 1);
  const bool tables = b.s->opt.use_dense && b.s->opt.dense && b.s->opt.probe_budget_x > 0;
  if (kProbeAnd && !b.exhaustive && tables && b.n_queries >= (uint32_t)b.s->opt.ashare_min_batch)
    b.and_probe = kProbeAnd >= 2 || (uint64_t)b.n_sparse2 * 10u >= b.n_queries;
  probe_begin_batch(b.s);  // (the probe pool's clock: tables this batch uses are not evicted for one another)
  if (b.exhaustive || !((knobs().use_bshare && b.n_bool_queries) || b.and_probe) || !tables) return TQ_OK;
  bool built = false;
  for (uint32_t qi = 0; qi < b.n_queries; ++qi) {
    const tq_query &q = b.queries[qi];
    // (2-term intersections of a batch large enough for the shared launch: the list that is probed — the
    // more frequent one — the same way; lists 2.. of longer intersections are reached through the term
    // table, which only knows a list's own tables)
    const bool and2 = b.and_probe && q.mode == TQ_MODE_AND && q.n_terms == 2;
    if (!((q.mode == TQ_MODE_BOOL && knobs().use_bshare) || and2) || !q.terms || q.n_terms > TQD_AS_MAX_TERMS || q.k > 128u) continue;
    uint32_t skip = 0xFFFFFFFFu;  // (the leader of an intersection is decoded, never probed)
    if (and2 && q.terms[0] < b.s->terms.size() && q.terms[1] < b.s->terms.size())
      skip = b.s->terms[q.terms[1]].doc_freq < b.s->terms[q.terms[0]].doc_freq ? 1u : 0u;
    for (uint32_t i = 0; i < q.n_terms; ++i) {
      if (i == skip) continue;
      const uint32_t h = q.terms[i];
      if (h >= b.s->terms.size()) continue;  // (absent, or reported by plan_query)
      const TermHost &th = b.s->terms[h];
      if (th.dense_blob && th.tf8_blob) continue;
      if (and2 && th.rdir_blob && b.s->rdir_span_ok) continue;  // (probed through its range directory)
      // (a list too short for a directory — rdir_plan — is too short for a max_doc / 4-byte slot of the probe pool:
      // its queries keep the per-query kernel, whose leader has at most as many blocks)
      if (and2 && b.s->opt.rdir_budget_x > 0 && th.doc_freq < 256u) continue;
      const bool had = th.probe_dense_blob && th.probe_tf8_blob;
      bool ok = false;
      const int prc = build_probe_tables(b.s, h, &ok);  // (tables it already has: marked as used by this batch)
      if (prc != TQ_OK) return prc;
      built = built || (ok && !had);
    }
  }
  if (built) b.s->share_span_terms = ~(size_t)0;  // (the tables' address span is taken again: count_leaders)
  return TQ_OK;
}

}  // namespace

// Nested boolean queries (tq_tree.hip) reach EVERY list through a bitmap, in both modes.
int build_tree_query_probe_tables(tq_segment *s, const tq_query &q, bool *built, bool flat_too) {
  if (!s->opt.use_dense || !s->opt.dense || s->opt.probe_budget_x <= 0) return TQ_OK;
  if (q.mode != TQ_MODE_BOOL || !q.terms || q.n_terms > TQ_MAX_TERMS || !(flat_too || bool_query_is_tree(q))) return TQ_OK;
  for (uint32_t i = 0; i < q.n_terms; ++i) {
    const uint32_t h = q.terms[i];
    if (h >= s->terms.size()) continue;
    const TermHost &th = s->terms[h];
    if (!(th.dense_blob && th.tf8_blob)) {
      const bool had = th.probe_dense_blob && th.probe_tf8_blob;
      bool ok = false;
      const int prc = build_probe_tables(s, h, &ok, true);
      if (prc != TQ_OK) return prc;
      *built = *built || (ok && !had);
    }
    // a term of a phrase inside the boolean query: its positions are reached from the bitmap's rank
    if (q.nested_occurs && q.nested_occurs[i] != 255u && (q.nested_occurs[i] & TQ_NESTED_PHRASE) &&
        !s->terms[h].posdir_blob && !s->terms[h].probe_posdir_blob) {
      bool ok = false;
      const int prc = build_probe_posdir(s, h, &ok);
      if (prc != TQ_OK) return prc;
      *built = *built || ok;
    }
  }
  return TQ_OK;
}

namespace {

int build_tree_probe_tables(Batch &b) {
  if (!b.n_bool_queries) return TQ_OK;
  bool built = false;
  for (uint32_t qi = 0; qi < b.n_queries; ++qi) {
    // (a flat query that names a term set takes the tree kernel too: its other lists get bitmaps the same way)
    const int prc = build_tree_query_probe_tables(b.s, b.queries[qi], &built, b.set_q && b.set_q[qi]);
    if (prc != TQ_OK) return prc;
  }
  if (built) b.s->share_span_terms = ~(size_t)0;
  return TQ_OK;
}

// ALL-BASED queries (tq_all.hip) reach every list through a bitmap too: the MustNot lists for their bits, the Should
// lists for bits, rank and tf bytes.  The probe pool's tables, no new kind.
int build_all_probe_tables(Batch &b) {
  if (!b.n_all_queries || !b.s->opt.use_dense || !b.s->opt.dense || b.s->opt.probe_budget_x <= 0) return TQ_OK;
  bool built = false;
  for (uint32_t qi = 0; qi < b.n_queries; ++qi) {
    const tq_query &q = b.queries[qi];
    if (!query_has_all(q)) continue;
    for (uint32_t i = 0; i < q.n_terms; ++i) {
      const uint32_t h = q.terms[i];
      if (h >= b.s->terms.size()) continue;  // (All, absent, or reported by plan_query)
      const TermHost &th = b.s->terms[h];
      if (th.dense_blob && th.tf8_blob) continue;
      const bool had = th.probe_dense_blob && th.probe_tf8_blob;
      bool ok = false;
      const int prc = build_probe_tables(b.s, h, &ok, true);
      if (prc != TQ_OK) return prc;
      built = built || (ok && !had);
    }
  }
  if (built) b.s->share_span_terms = ~(size_t)0;
  return TQ_OK;
}

// Which list would lead an AND query in the shared-intersection launch (0xFFFFFFFF: the query does not qualify).
uint32_t ashare_leader(const Batch &b, const tq_query &q, uint32_t cache_idx) {
  if (q.mode != TQ_MODE_AND || q.n_terms < 2 || q.n_terms > TQD_AS_MAX_TERMS || q.k == 0 || q.k > 128u ||
      !q.terms || !q.weights || cache_idx >= 256u)
    return 0xFFFFFFFFu;
  uint32_t best = 0xFFFFFFFFu, best_i = 0;
  for (uint32_t i = 0; i < q.n_terms; ++i) {
    if (q.terms[i] == TQ_TERM_ABSENT || q.terms[i] >= b.s->terms.size() || !(q.weights[i] >= 0.0f)) return 0xFFFFFFFFu;
    const uint32_t df = b.s->terms[q.terms[i]].doc_freq;
    if (df < best) {  // (first of the rarest: what the stable sort by doc freq puts in front)
      best = df;
      best_i = i;
    }
  }
  for (uint32_t i = 0; i < q.n_terms; ++i) {
    if (i == best_i) continue;
    const TermHost &th = b.s->terms[q.terms[i]];
    if (!(th.dense_blob && th.tf8_blob) && !(q.n_terms == 2 && th.rdir_blob && b.s->rdir_span_ok) &&
        !(b.and_probe && q.n_terms == 2 && th.probe_dense_blob && th.probe_tf8_blob))
      return 0xFFFFFFFFu;
  }
  return q.terms[best_i];
}

// Queries per shared-intersection leader, the "ashare_min_batch" gate, the AND tile cap, each distinct list's bytes once.
void count_leaders(Batch &b) {
  PlanScratch &ps = *b.ps;
  update_table_span(b.s);  // (probe tables built by the pre-pass moved it)
  b.ashare_on = knobs().use_ashare && !b.exhaustive && b.s->d_docmat && b.s->opt.use_dense && b.s->share_span_ok;
  b.ashare_and = b.ashare_on && !b.co.no_ashare;  // (intersections: also needs "ashare_min_batch" qualifying queries)
  uint64_t and_lead_blocks = 0;  // leader blocks of the batch's intersections (sizes their tiles below)
  if (ps.term_stamp.size() < 2 * b.s->terms.size()) ps.term_stamp.resize(2 * b.s->terms.size(), 0u);
  if (++ps.batch_stamp == 0u) {
    std::fill(ps.term_stamp.begin(), ps.term_stamp.end(), 0u);
    ps.batch_stamp = 1u;
  }
  ps.and_lead_count.assign(b.ashare_on ? b.s->terms.size() : 0, 0u);
  ps.q_leader.resize(b.ashare_on ? b.n_queries : 0);
  for (uint32_t qi = 0; qi < b.n_queries; ++qi) {
    const tq_query &q = b.queries[qi];
    if (!q.terms || q.n_terms > TQ_MAX_TERMS) continue;  // (reported by plan_query)
    uint32_t lead_blocks = 0xFFFFFFFFu;
    for (uint32_t i = 0; i < q.n_terms; ++i) {
      const uint32_t h = q.terms[i];
      if (h >= b.s->terms.size()) continue;
      lead_blocks = std::min(lead_blocks, b.s->terms[h].n_blocks);
      if (ps.term_stamp[2 * h] != ps.batch_stamp) {
        ps.term_stamp[2 * h] = ps.batch_stamp;
        b.unique_bytes += b.s->terms[h].postings_len;
      }
      if (q.mode == TQ_MODE_PHRASE && ps.term_stamp[2 * h + 1] != ps.batch_stamp) {
        ps.term_stamp[2 * h + 1] = ps.batch_stamp;
        b.unique_bytes += b.s->terms[h].positions_len;
      }
    }
    if (q.mode == TQ_MODE_AND && q.n_terms >= 2 && lead_blocks != 0xFFFFFFFFu) and_lead_blocks += lead_blocks;
    if (b.ashare_on) {
      const uint32_t lh = ashare_leader(b, q, ps.q_cache[qi]);
      ps.q_leader[qi] = lh;
      if (lh != 0xFFFFFFFFu) ++ps.and_lead_count[lh];
    }
  }
  if (b.ashare_on) {  // a small batch keeps the per-query kernels ("ashare_min_batch")
    static const uint32_t kMinBatchEnv = tune_u32("TQ_AS_MIN_BATCH", 0xFFFFFFFFu);
    const uint32_t min_batch = kMinBatchEnv != 0xFFFFFFFFu ? kMinBatchEnv : (uint32_t)b.s->opt.ashare_min_batch;
    uint32_t n_el = 0;
    for (uint32_t qi = 0; qi < b.n_queries && n_el < min_batch; ++qi) {
      const uint32_t lh = ps.q_leader[qi];
      if (lh != 0xFFFFFFFFu && ps.and_lead_count[lh] >= knobs().ashare_min) ++n_el;
    }
    b.ashare_and = n_el >= min_batch;
  }
  // Tiles of the per-query intersection kernel: 64 leader blocks — unless the whole batch would then be a few hundred
  // wavefronts walking their tiles serially (one query over a 250 k-doc leader = 31 wavefronts x 64 blocks = 0.23 of
  // a 0.27 ms call): a batch of fewer than kSmallBatchBlocks leader blocks (one to four queries) is cut into about
  // kSmallBatchTiles tiles of at least kMinTileBlocks blocks, and the hundreds of partial lists that makes are merged in
  // two levels (tqk_launch_merge).  One query per call: 0.27 -> 0.14 ms.
  static const uint32_t kSmallBatchTiles = std::max<uint32_t>(1u, tune_u32("TQ_AND_SMALL_TILES", 2048));
  static const uint32_t kMinTileBlocks = std::min<uint32_t>(TQD_AND_TILE, std::max<uint32_t>(1u, tune_u32("TQ_AND_MIN_TILE", 4)));
  static const uint64_t kSmallBatchBlocks = tune_u32("TQ_AND_SMALL_BLOCKS", 8192);  // (tq_plan_chunks.cpp: the chunk floor follows)
  b.and_tile_cap = and_lead_blocks < kSmallBatchBlocks
                       ? (uint32_t)std::min<uint64_t>(TQD_AND_TILE, std::max<uint64_t>(kMinTileBlocks, and_lead_blocks / kSmallBatchTiles))
                       : TQD_AND_TILE;
}

// The leaders of this batch's shared-intersection launch get their norm bytes in posting order (build_lnorm, tq_terms.cpp)
// the first time they lead: a launch each on the batch's stream, ahead of the batch's kernels.
// ... and their doc-matrix words in posting order (plan_lmat: allocated and named here, filled by fill_leader_mats).
void build_leader_norms(Batch &b) {
  tq_segment *s = b.s;
  s->lmat_stale_skips = 0;
  if (b.ashare_and) {
    const PlanScratch &ps = *b.ps;
    const bool norms = s->dseg.fieldnorm != nullptr;
    for (size_t h = 0; h < ps.and_lead_count.size(); ++h) {
      if (ps.and_lead_count[h] < knobs().ashare_min) continue;
      if (norms && !s->terms[h].lnorm_blob) build_lnorm(s, (uint32_t)h, b.st);
      bool fill = false;
      if (plan_lmat(s, (uint32_t)h, &fill) && fill) b.lmat_fill.push_back((uint32_t)h);
    }
    update_table_span(s);  // (new tables moved it; share_span_ok decided the batch's route before they existed)
  }
  s->docmat_epoch_planned = s->docmat_epoch;
}

// One query's routing: its descriptor and the launch group it joins.
struct Route {
  TqdQuery dq{};
  int group = kGUnion;
  uint32_t n_tiles = 0, tile_cost = 1;
  uint64_t qbytes = 0;
};

// The arguments of a query the device path does not take.
int check_query(const Batch &b, uint32_t qi) {
  const tq_query &q = b.queries[qi];
  if (q.n_terms == 0 || q.n_terms > TQ_MAX_TERMS)
    return fail(TQ_ERR_INVALID, "query %u: n_terms %u not in 1..%u", qi, q.n_terms, TQ_MAX_TERMS);
  if (q.k == 0 || q.k > TQ_MAX_K || q.k > b.out_stride)
    return fail(TQ_ERR_INVALID, "query %u: k %u not in 1..min(%u, out_stride %u)", qi, q.k,
                TQ_MAX_K, b.out_stride);
  if (!q.terms || !q.weights || !q.tf_cache)
    return fail(TQ_ERR_INVALID, "query %u: null terms/weights/tf_cache", qi);
  if (q.mode > TQ_MODE_BOOL) return fail(TQ_ERR_INVALID, "query %u: bad mode", qi);
  if (q.mode == TQ_MODE_BOOL && !q.occurs)
    return fail(TQ_ERR_INVALID, "query %u: TQ_MODE_BOOL needs occurs", qi);
  if (q.mode == TQ_MODE_PHRASE && (q.n_terms < 2 || !q.phrase_offsets))
    return fail(TQ_ERR_INVALID, "query %u: a phrase needs >= 2 terms and offsets", qi);
  if (q.mode == TQ_MODE_PHRASE && q.n_terms > 8)
    return fail(TQ_ERR_UNSUPPORTED, "query %u: device phrases take at most 8 terms", qi);
  // NaN / inf weights (boosts) would break the total order of the top-k keys and of merge_top_k
  for (uint32_t i = 0; i < (q.mode == TQ_MODE_PHRASE ? 1u : q.n_terms); ++i)
    if (!std::isfinite(q.weights[i]))
      return fail(TQ_ERR_INVALID, "query %u: weight %u is not finite", qi, i);
  for (uint32_t i = 0; i < q.n_terms; ++i)
    if (q.terms[i] != TQ_TERM_ABSENT && q.terms[i] != TQ_TERM_ALL && q.terms[i] >= b.s->terms.size())
      return fail(TQ_ERR_INVALID, "query %u: unknown term handle %u", qi, q.terms[i]);
  return TQ_OK;
}

// The lists of an intersection / phrase by doc_freq ascending, stable (block_wand_intersection.rs:26-29 / intersection.rs:93).
int sort_by_doc_freq(const Batch &b, uint32_t qi, Route &r) {
  const tq_query &q = b.queries[qi];
  const bool phrase = q.mode == TQ_MODE_PHRASE;
  uint32_t order[TQ_MAX_TERMS];
  for (uint32_t i = 0; i < q.n_terms; ++i) order[i] = i;
  small_stable_sort(order, order + q.n_terms, [&](uint32_t x, uint32_t y) {
    return b.s->terms[q.terms[x]].doc_freq < b.s->terms[q.terms[y]].doc_freq;
  });
  uint32_t max_off = 0;
  if (phrase)
    for (uint32_t i = 0; i < q.n_terms; ++i) max_off = std::max(max_off, q.phrase_offsets[i]);
  for (uint32_t i = 0; i < q.n_terms; ++i) {
    const uint32_t src = order[i];
    r.dq.term[i] = q.terms[src];
    r.dq.weight[i] = phrase ? q.weights[0] : q.weights[src];
    r.qbytes += b.s->terms[q.terms[src]].postings_len;
    if (phrase) {
      r.dq.phrase_off[i] = max_off - q.phrase_offsets[src];
      if (b.s->terms[q.terms[src]].positions_len == 0)
        return fail(TQ_ERR_UNSUPPORTED, "query %u: phrase on a field without positions", qi);
      r.qbytes += b.s->terms[q.terms[src]].positions_len;
    }
  }
  r.dq.n_terms = q.n_terms;
  return TQ_OK;
}

// An intersection of two or more lists: the shared-intersection launch, or leader-block tiles of the per-query kernel.
void route_and(const Batch &b, uint32_t qi, Route &r, RouteTotals &t) {
  const tq_query &q = b.queries[qi];
  TqdQuery &dq = r.dq;
  // cost of one leader block: its own decode + the distinct blocks of the non-dense
  // lists its 128 candidates can fall into (each decoded by the whole wave, serially)
  const uint32_t lead_blocks = b.s->terms[dq.term[0]].n_blocks;
  uint32_t c_lb = 1;
  bool all_dense = true;
  for (uint32_t i = 1; i < q.n_terms; ++i) {
    const TermHost &th = b.s->terms[dq.term[i]];
    if (th.dense_blob && b.s->opt.use_dense) continue;
    all_dense = false;
    c_lb += 2u * std::min<uint32_t>(128u, (th.n_blocks + lead_blocks - 1) / lead_blocks);
  }
  static const uint32_t kAndTileNum = std::max<uint32_t>(1u, tune_u32("TQ_AND_TILE_NUM", TQD_AND_TILE));
  dq.tile_blocks = std::min<uint32_t>(b.and_tile_cap, std::max<uint32_t>(1u, kAndTileNum / c_lb));
  r.tile_cost = dq.tile_blocks * c_lb;
  r.n_tiles = (lead_blocks + dq.tile_blocks - 1) / dq.tile_blocks;
  r.group = all_dense ? kGAndDense : kGAnd;
  bool nonneg = true;
  for (uint32_t i = 0; i < q.n_terms; ++i) nonneg = nonneg && dq.weight[i] >= 0.0f;
  bool ashare = false;
  if (b.ashare_and && nonneg && (all_dense || q.n_terms == 2)) {  // (2 lists: list 1 may have probe tables, q_leader knows)
    const uint32_t lh = b.ps->q_leader[qi];
    ashare = lh != 0xFFFFFFFFu && lh == dq.term[0] && b.ps->and_lead_count[lh] >= knobs().ashare_min;
  }
  if (ashare) {  // (planned per leader, not per query: build_ashare_plan)
    dq.flags |= TQD_QF_PRUNE;
    dq.thr_index = t.n_thr_rows;
    t.n_thr_rows += q.k <= 16u ? 1u : 4u;  // 64 hashed score slots for k <= 16, 256 above
    r.n_tiles = 0;
    r.group = kGAShare;
    t.n_ashare_ext += q.n_terms > 2u ? 1u : 0u;
  } else if (!b.exhaustive && nonneg) {  // block-max bounds need weights >= 0
    dq.flags |= TQD_QF_PRUNE;
    // the shared threshold pays off on long lists only; k-th largest of 64 slots needs k <= 64
    if (q.k <= TQD_THR_SLOTS && r.n_tiles >= 2) dq.thr_index = t.n_thr_rows++;
  }
}

// A phrase: leader-block tiles like AND, every match also walks its positions — or the bitmap-AND sweep.
void route_phrase(const Batch &b, uint32_t qi, Route &r, RouteTotals &t) {
  const tq_query &q = b.queries[qi];
  TqdQuery &dq = r.dq;
  // phrases whose lists ALL have a bitmap, byte-wide tfs and a position directory, the rarest one
  // still about a posting per bitmap word: the bitmap-AND sweep (phrase_sweep_kernel)
  static const uint32_t kPhSweepRatio = tune_u32("TQ_PH_SWEEP_RATIO", 128);  // 0 = never (64 until round 6: with leaders down to max_doc / 128 the realistic phrase stream ran 10 % faster)
  const uint32_t lead_blocks = b.s->terms[dq.term[0]].n_blocks;
  bool ph_sweep = kPhSweepRatio && q.n_terms <= 4u && b.s->opt.use_dense &&
                  (uint64_t)b.s->terms[dq.term[0]].doc_freq * kPhSweepRatio >= b.s->max_doc;
  for (uint32_t i = 0; ph_sweep && i < q.n_terms; ++i) {
    const TermHost &th = b.s->terms[dq.term[i]];
    if (!(th.dense_blob && th.tf8_blob && th.posdir_blob)) ph_sweep = false;
  }
  // the lean instantiation needs a bitmap, a doc-matrix column and a position directory
  // for every non-leader list
  for (uint32_t i = 1; !ph_sweep && i < q.n_terms; ++i) {
    const TermHost &th = b.s->terms[dq.term[i]];
    const bool col = ((b.s->h_dterms[dq.term[i]].has_freq >> 8) & 0xFFu) != 0u;
    if (!(th.dense_blob && th.posdir_blob && th.tf8_blob && col && b.s->opt.use_dense && b.s->d_docmat))
      t.phrase_all_dense = false;
  }
  // (64-block tiles: one leader block per lane of the pre-filter; 32 was 10 % slower)
  static const uint32_t kPhTile = std::min<uint32_t>(TQD_AND_TILE, std::max<uint32_t>(1u, tune_u32("TQ_PH_TILE_BLOCKS", 64)));
  dq.tile_blocks = kPhTile;
  r.tile_cost = 2u * kPhTile;
  r.n_tiles = (lead_blocks + dq.tile_blocks - 1) / dq.tile_blocks;
  r.group = kGPhrase;
  if (ph_sweep) {  // tiles are runs of 2048 bitmap words (phrase_sweep_kernel's SWEEP_WORDS)
    const uint32_t n_words = (b.s->max_doc + 31u) / 32u;
    r.n_tiles = (n_words + 2047u) / 2048u;
    r.tile_cost = 64u;
    r.group = kGPhSweep;
  }
  // A phrase matches a doc at most min(tf of its terms) times: bm25(sum of idfs, norm, min tf) bounds the doc's
  // score BEFORE its positions are read.  The reference filters finished scores only (weight.rs:47-60); with
  // the query's threshold shared across its wavefronts (the slots of the other pruned kernels) the phrase
  // kernels skip the position walk of every candidate that cannot reach the top-k — the same top-k, bit for bit
  // (candidates EQUAL to the bound are walked: ties resolve by doc id).
  static const bool kPhPrune = tune_u32("TQ_PH_PRUNE", 1) != 0;
  if (kPhPrune && !b.exhaustive && q.weights[0] >= 0.0f && q.k <= TQD_THR_SLOTS) {
    dq.flags |= TQD_QF_PRUNE;
    dq.thr_index = t.n_thr_rows++;
  }
}

}  // namespace

int fail_tree_tables(const tq_segment *s, uint32_t qi) {
  return fail(TQ_ERR_UNSUPPORTED,
              "query %u: nested boolean queries need the lists' bitmaps (\"use_dense\" %d, one 32 GB table span: %s — tables from %llx, arena %llx + %zu MB "
              "mapped, %zu allocations outside it)",
              qi, (int)s->opt.use_dense, s->share_span_ok ? "ok" : "exceeded", (unsigned long long)s->share_table_lo, (unsigned long long)(uintptr_t)s->dense_arena,
              s->dense_arena_mapped >> 20, s->dense_extra.size());
}

namespace {

// A clause that is itself a BooleanQuery of terms (tq_query.nested_occurs): evaluated over bitmaps, tq_tree.hip.
int route_tree(const Batch &b, uint32_t qi, Route &r, Group &tree_group) {
  if (!b.s->share_span_ok || !b.s->opt.use_dense) return fail_tree_tables(b.s, qi);
  TqdTreeQuery tq;
  const int rc = plan_tree_query(b.s, b.queries[qi], qi, tq, r.qbytes, b.s->share_table_lo);
  if (rc != TQ_OK) return rc;
  tq.cache_idx = r.dq.cache_idx;
  tree_group.tree.push_back(tq);
  r.dq.n_terms = tq.n_terms;
  r.n_tiles = 0;
  r.group = kGTree;
  return TQ_OK;
}

// A TQ_MODE_PHRASE query with slop > 0 (its view: strip_all_clauses): a launch group of its own, tq_phrase_slop.hip.
int route_slop(const Batch &b, uint32_t qi, Route &r, Group &slop_group) {
  if (!b.s->share_span_ok || !b.s->opt.use_dense) return fail_tree_tables(b.s, qi);
  TqdSlopQuery sq;
  r.qbytes = 0;
  const int rc = plan_slop_query(b.s, b.queries[qi], qi, b.slop_q[qi], sq, r.qbytes, false);
  if (rc != TQ_OK) return rc;
  sq.cache_idx = r.dq.cache_idx;
  slop_group.slop.push_back(sq);
  r.dq.n_terms = sq.n_terms;
  r.n_tiles = 0;
  r.group = kGSlop;
  return TQ_OK;
}

// A query whose AllQuery clauses make every doc a candidate (tq_all.cpp: ALL-BASED; strip_all_clauses has replaced the
// EMPTY and PLAIN ones by their views): the Should lists in score-sum order, then the MustNot lists, over bitmaps.
int route_all(const Batch &b, uint32_t qi, Route &r, Group &all_group) {
  const tq_query &q = b.queries[qi];
  FlatClauses fc;
  const char *why = "";
  const int prc = parse_flat_clauses(b.s, q, fc, &why);
  if (prc != FLAT_OK) return fail(prc == FLAT_UNSUPPORTED ? TQ_ERR_UNSUPPORTED : TQ_ERR_INVALID, "query %u: %s", qi, why);
  TqdAllQuery aq{};
  aq.k = q.k;
  aq.cache_idx = r.dq.cache_idx;
  aq.min_should = fc.msm;
  memcpy(&aq.base_bits, &fc.all_base, sizeof(float));
  if (aq.min_should > 15u) return fail(TQ_ERR_UNSUPPORTED, "query %u: minimum_number_should_match above 15", qi);
  uint32_t n = 0;
  for (uint32_t pass = 0; pass < 2; ++pass) {
    for (uint32_t c = 0; c < fc.n_cl; ++c) {
      const FlatClauses::Clause &C = fc.cl[c];
      if (C.occur != (pass == 0 ? (uint32_t)TQ_SHOULD : (uint32_t)TQ_MUST_NOT)) continue;
      for (uint32_t i = 0; i < C.n; ++i) {
        const TermHost &th = b.s->terms[C.terms[i]];
        const bool own = th.dense_blob && th.tf8_blob;
        // (a term set: a MustNot list here — strip_all_clauses — of which all_kernel reads the bits alone)
        const bool cset = th.set_kind == TermHost::kSet && pass == 1;
        const void *bm = cset || own ? th.dense_blob : th.probe_dense_blob, *t8 = cset ? th.dense_blob : own ? th.tf8_blob : th.probe_tf8_blob;
        if (!b.s->share_span_ok || !b.s->opt.use_dense || !bm || !t8)
          return fail(TQ_ERR_UNSUPPORTED,
                      "query %u: a query with a match-all clause names a list without a bitmap (options \"dense\" / \"use_dense\" / \"probe_budget_x\" off, "
                      "a list whose tables did not fit \"dense_budget_x\", or the tables span more than 32 GB)", qi);
        aq.dense_off[n] = (uint32_t)(((uint64_t)bm - b.s->share_table_lo) >> 3);
        aq.tf8_off[n] = (uint32_t)(((uint64_t)t8 - b.s->share_table_lo) >> 3);
        memcpy(&aq.weight_bits[n], &q.weights[C.pos[i]], sizeof(float));
        aq.handle[n] = C.terms[i];
        if (pass == 0 && i + 1 == C.n) aq.clause_end |= 1u << n;
        ++n;
      }
    }
    if (pass == 0) aq.n_should = n;
  }
  aq.n_lists = n;
  // Without a list and without deletes the top-k is the first k docs: their tiles alone; the other docs are counted here.
  const uint32_t n_words = (b.s->max_doc + 31u) / 32u, tiles = tqk_all_tiles(n_words);
  aq.n_tiles = tiles;
  if (n == 0 && !b.s->d_alive) aq.n_tiles = std::min<uint32_t>(tiles, (q.k + TQK_ALL_TILE_WORDS * 32u - 1u) / (TQK_ALL_TILE_WORDS * 32u));
  const uint64_t scanned_docs = std::min<uint64_t>(b.s->max_doc, (uint64_t)aq.n_tiles * TQK_ALL_TILE_WORDS * 32u);
  aq.extra_matches = (uint32_t)(b.s->max_doc - scanned_docs);
  r.qbytes += (scanned_docs + 31u) / 32u * (8ull * n + (b.s->d_alive ? 4u : 0u));  // the HBM model of tq_all.hip
  all_group.all.push_back(aq);
  r.dq.n_terms = n;
  r.dq.n_parts = aq.n_tiles;
  r.n_tiles = 0;
  r.group = kGAll;
  return TQ_OK;
}

// A boolean query of terms: the union kernel's BOOL instantiation, or the shared launch (tq_ashare.hip, boolean leads)
// when every list is reached through its bitmap and tf bytes (the only list of a lead set of one is only decoded).
int route_bool(const Batch &b, uint32_t qi, Route &r, RouteTotals &t) {
  const tq_query &q = b.queries[qi];
  TqdQuery &dq = r.dq;
  const int rc = plan_bool_query(b.s, q, qi, dq, r.qbytes, r.n_tiles, r.tile_cost, t.n_thr_rows, b.exhaustive);
  if (rc != TQ_OK) return rc;
  bool bshare = knobs().use_bshare && !b.co.no_bshare && b.ashare_on && (dq.flags & TQD_QF_PRUNE) && dq.thr_index != 0xFFFFFFFFu && dq.n_terms >= 1 &&
                dq.n_terms <= TQD_AS_MAX_TERMS && q.k <= 128u && dq.cache_idx < 256u && dq.n_lead >= 1;
  for (uint32_t i = 0; bshare && i < dq.n_terms; ++i) {
    const TermHost &th = b.s->terms[dq.term[i]];
    if (!(th.dense_blob && th.tf8_blob) && !(th.probe_dense_blob && th.probe_tf8_blob) && !(knobs().bs_rdir && th.rdir_blob && b.s->rdir_span_ok) &&
        !(dq.n_lead == 1 && i == 0))
      bshare = false;
  }
  r.group = bshare ? kGBShare : kGBool;
  return TQ_OK;
}

// Pure unions, NOT pruned, k <= 128, <= 8 terms, positive weights, whose lists together hold at least 1/dense_ratio of
// the segment: the doc-major launch (tq_xunion.hip) — up to 256 distinct lists and 8192 queries per batch, one
// Bm25Weight cache; the rest keeps the window kernel.
int route_xunion(const Batch &b, Route &r, const Group &xunion_group, const tq_query &q, RouteTotals &t) {
  PlanScratch &ps = *b.ps;
  TqdQuery &dq = r.dq;
  // (a batch with fewer unions than the launch needs never builds plain lists for it: those stay
  // charged to the segment's table budget for good — ADVICE r03)
  bool dense_u = b.dense_ratio && b.n_union_queries >= b.dense_min_queries && b.exhaustive && b.s->opt.use_dense && dq.n_terms >= 1 && dq.n_terms <= 8 &&
            q.k <= 128 && (ps.xcache == 0xFFFFFFFFu || ps.xcache == dq.cache_idx) &&
            xunion_group.queries.size() < TQK_XU_MAX_QUERIES;
  uint64_t sum_df = 0;
  uint32_t new_rows = 0;
  for (uint32_t i = 0; dense_u && i < dq.n_terms; ++i) {
    if (!(dq.weight[i] > 0.0f)) dense_u = false;
    sum_df += b.s->terms[dq.term[i]].doc_freq;
    bool seen = ps.xrow_of.count(xrow_key(dq.term[i], dq.weight[i])) != 0;
    for (uint32_t j = 0; j < i; ++j) seen = seen || (dq.term[j] == dq.term[i] && dq.weight[j] == dq.weight[i]);
    if (!seen) ++new_rows;
  }
  if (dense_u && (sum_df * b.dense_ratio < b.s->max_doc || ps.xrow_term.size() + new_rows > TQK_XU_MAX_ROWS - 1u))
    dense_u = false;
  for (uint32_t i = 0; dense_u && i < dq.n_terms; ++i) {
    const TermHost &th = b.s->terms[dq.term[i]];
    if (th.dense_blob && th.tf8_blob) continue;
    bool ok = false;
    const int frc = build_flat(b.s, dq.term[i], b.st, &ok);
    if (frc != TQ_OK) return frc;
    if (!ok) dense_u = false;
  }
  if (!dense_u) return TQ_OK;
  ps.xcache = dq.cache_idx;
  for (uint32_t i = 0; i < dq.n_terms; ++i) {
    const uint64_t key = xrow_key(dq.term[i], dq.weight[i]);
    if (ps.xrow_of.emplace(key, (uint32_t)ps.xrow_term.size()).second) ps.xrow_term.push_back(key);
  }
  dq.thr_index = t.n_thr_rows;
  t.n_thr_rows += 4u;
  r.group = kGXUnion;
  return TQ_OK;
}

// A union (or a one-list intersection): shared-union, doc-major, 4096-doc windows, or candidate-driven tiles.
int route_union(const Batch &b, uint32_t qi, Route &r, Group *groups, RouteTotals &t) {
  const tq_query &q = b.queries[qi];
  TqdQuery &dq = r.dq;
  uint32_t n = 0;
  for (uint32_t i = 0; i < q.n_terms; ++i) {
    if (q.terms[i] == TQ_TERM_ABSENT) continue;  // (TermWeight::for_each_pruning for one list: every doc of it)
    dq.term[n] = q.terms[i];
    dq.weight[n] = q.weights[i];
    r.qbytes += b.s->terms[q.terms[i]].postings_len;
    ++n;
  }
  dq.n_terms = n;
  // terms by weight descending (stable): the score sum order of the union kernel, and what
  // makes the low-weight (dense) lists the non-essential suffix of MaxScore pruning
  uint32_t order[TQ_MAX_TERMS];
  for (uint32_t i = 0; i < n; ++i) order[i] = i;
  small_stable_sort(order, order + n, [&](uint32_t x, uint32_t y) { return dq.weight[x] > dq.weight[y]; });
  uint32_t t2[TQ_MAX_TERMS];
  float w2[TQ_MAX_TERMS];
  for (uint32_t i = 0; i < n; ++i) {
    t2[i] = dq.term[order[i]];
    w2[i] = dq.weight[order[i]];
  }
  bool nonneg = true;
  for (uint32_t i = 0; i < n; ++i) {
    dq.term[i] = t2[i];
    dq.weight[i] = w2[i];
    nonneg = nonneg && w2[i] >= 0.0f;
  }
  if (!b.exhaustive && nonneg && n) {
    dq.flags |= TQD_QF_PRUNE;
    if (q.k <= 2 * TQD_THR_SLOTS) {  // k-th largest of 64 (128) slots needs k <= 64 (128)
      dq.thr_index = t.n_thr_rows;
      t.n_thr_rows += 4u;  // union kernel: 64 slots for k <= 16, 256 above; the window kernel 64 / 128
    }
  }
  bool share = knobs().use_ushare && b.s->share_span_ok && !b.or_windows && (dq.flags & TQD_QF_PRUNE) && dq.thr_index != 0xFFFFFFFFu &&
               n >= 1 && n <= TQD_US_MAX_TERMS && b.s->d_docmat && b.s->opt.use_dense && dq.cache_idx < 256u;
  for (uint32_t i = 0; share && i < n; ++i)  // (lists with a bitmap carry byte-wide tfs)
    if (b.s->terms[dq.term[i]].dense_blob && !b.s->terms[dq.term[i]].tf8_blob) share = false;
  if (share) {  // (planned per term, not per query: build_share_plan)
    r.group = kGUShare;
  } else if (b.or_windows) {
    uint32_t max_last = 0;
    for (uint32_t i = 0; i < n; ++i) max_last = std::max(max_last, b.s->terms[dq.term[i]].last_doc);
    if (n) r.n_tiles = max_last / TQD_OR_WINDOW + 1;
    if (b.exhaustive) return route_xunion(b, r, groups[kGXUnion], q, t);  // (never pruned: never planned by the slab threads)
  } else if (n) {
    // candidate-driven: every list leads its own run of tiles; a candidate probes all the
    // other lists (non-dense ones cost a seek + a block search)
    uint32_t sparse = 0;
    for (uint32_t i = 0; i < n; ++i)
      if (!(b.s->terms[dq.term[i]].dense_blob && b.s->opt.use_dense)) ++sparse;
    const uint32_t c_lb = 1u + n + 8u * sparse;
    static const uint32_t kOrTileBlocks = tune_u32("TQ_OR_TILE_BLOCKS", 0);
    static const uint32_t kOrTileNum = std::max<uint32_t>(1u, tune_u32("TQ_OR_TILE_NUM", TQD_AND_TILE * 2u));
    dq.tile_blocks = kOrTileBlocks ? std::min<uint32_t>(kOrTileBlocks, TQD_AND_TILE)
                                   : std::min<uint32_t>(TQD_AND_TILE, std::max<uint32_t>(1u, kOrTileNum / c_lb));
    r.tile_cost = dq.tile_blocks * c_lb;
    uint32_t acc_tiles = 0;
    for (uint32_t i = 0; i < n; ++i) {
      dq.lead_tile_start[i] = acc_tiles;
      acc_tiles += (b.s->terms[dq.term[i]].n_blocks + dq.tile_blocks - 1) / dq.tile_blocks;
    }
    for (uint32_t i = n; i <= TQ_MAX_TERMS; ++i) dq.lead_tile_start[i] = acc_tiles;
    dq.n_lead = n;
    r.n_tiles = acc_tiles;
  }
  return TQ_OK;
}

// One query -> its descriptor in its launch group.  Writes only to the groups / totals it is handed (the slab threads
// plan into groups of their own), and to the doc-major row table, which unpruned (never slabbed) batches alone use.
int plan_query(const Batch &b, uint32_t qi, Group *groups, RouteTotals &t) {
  int rc = check_query(b, qi);
  if (rc != TQ_OK) return rc;
  const tq_query &q = b.queries[qi];
  Route r;
  r.dq.thr_index = 0xFFFFFFFFu;
  r.dq.k = q.k;
  r.dq.cache_idx = b.ps->q_cache[qi];
  r.qbytes = 8ull * q.k;
  const bool any_absent = std::find(q.terms, q.terms + q.n_terms, TQ_TERM_ABSENT) != q.terms + q.n_terms;
  if (b.slop_q && b.slop_q[qi]) {
    rc = route_slop(b, qi, r, groups[kGSlop]);
  } else if (b.n_all_queries && query_has_all(q)) {
    rc = route_all(b, qi, r, groups[kGAll]);
  } else if (b.set_q && b.set_q[qi]) {  // (a TQ_MODE_BOOL view, whatever the caller's mode was)
    rc = route_tree(b, qi, r, groups[kGTree]);
  } else if (q.mode == TQ_MODE_BOOL) {
    rc = bool_query_is_tree(q) ? route_tree(b, qi, r, groups[kGTree]) : route_bool(b, qi, r, t);
  } else if (q.mode == TQ_MODE_OR || (q.mode == TQ_MODE_AND && q.n_terms == 1 && !any_absent)) {
    rc = route_union(b, qi, r, groups, t);
  } else if (any_absent) {  // an intersection / phrase with an absent list: no lists, no tiles, nothing matches
    r.group = q.mode == TQ_MODE_AND ? kGAndDense : kGPhrase;
  } else {
    rc = sort_by_doc_freq(b, qi, r);
    if (rc == TQ_OK && q.mode == TQ_MODE_AND) route_and(b, qi, r, t);
    if (rc == TQ_OK && q.mode == TQ_MODE_PHRASE) route_phrase(b, qi, r, t);
  }
  if (rc != TQ_OK) return rc;
  t.algo_bytes += r.qbytes;
  r.dq.n_tiles = r.n_tiles;
  r.dq.mode = (uint32_t)kGroupTraits[r.group].mode;
  Group &g = groups[r.group];
  g.queries.push_back(r.dq);
  g.tile_cost.push_back(r.tile_cost);
  g.out_index.push_back(qi);
  g.max_k = std::max(g.max_k, q.k);
  return TQ_OK;
}

// Slabs of a large pruned batch planned by the planner's threads, then laid end to end (slab order = query order).
int route_in_slabs(Batch &b, uint32_t q_slabs) {
  std::vector<QuerySlab> &qs = b.ps->q_slabs;
  if (qs.size() < q_slabs) qs.resize(q_slabs);
  parallel_slabs(q_slabs, [&](uint32_t sb) {
    QuerySlab &Q = qs[sb];
    for (int gi = 0; gi < kNGroups; ++gi) {
      Q.groups[gi].reset();
      Q.groups[gi].mode = kGroupTraits[gi].mode;
    }
    Q.t = RouteTotals{};
    Q.rc = TQ_OK;
    const uint32_t q0 = (uint32_t)((uint64_t)b.n_queries * sb / q_slabs), q1 = (uint32_t)((uint64_t)b.n_queries * (sb + 1) / q_slabs);
    for (uint32_t qi = q0; qi < q1; ++qi) {
      Q.rc = plan_query(b, qi, Q.groups, Q.t);
      if (Q.rc != TQ_OK) {
        Q.err = g_last_error;  // (this thread's slot: handed to the caller's below)
        break;
      }
    }
  });
  uint32_t thr_base[9] = {0};
  size_t g_base[kNGroups][9] = {};
  for (uint32_t sb = 0; sb < q_slabs; ++sb) {
    if (qs[sb].rc != TQ_OK) {
      g_last_error = qs[sb].err;
      return qs[sb].rc;
    }
    thr_base[sb + 1] = thr_base[sb] + qs[sb].t.n_thr_rows;
    b.t.algo_bytes += qs[sb].t.algo_bytes;
    b.t.n_ashare_ext += qs[sb].t.n_ashare_ext;
    b.t.phrase_all_dense = b.t.phrase_all_dense && qs[sb].t.phrase_all_dense;
    for (int gi = 0; gi < kNGroups; ++gi) g_base[gi][sb + 1] = g_base[gi][sb] + qs[sb].groups[gi].queries.size();
  }
  b.t.n_thr_rows = thr_base[q_slabs];
  for (int gi = 0; gi < kNGroups; ++gi) {
    Group &g = b.groups[gi];
    const size_t total = g_base[gi][q_slabs];
    g.queries.resize(total);
    g.tile_cost.resize(total);
    g.out_index.resize(total);
    for (uint32_t sb = 0; sb < q_slabs; ++sb) g.max_k = std::max(g.max_k, qs[sb].groups[gi].max_k);
    for (uint32_t sb = 0; sb < q_slabs; ++sb) g.tree.insert(g.tree.end(), qs[sb].groups[gi].tree.begin(), qs[sb].groups[gi].tree.end());
    for (uint32_t sb = 0; sb < q_slabs; ++sb) g.all.insert(g.all.end(), qs[sb].groups[gi].all.begin(), qs[sb].groups[gi].all.end());
    for (uint32_t sb = 0; sb < q_slabs; ++sb) g.slop.insert(g.slop.end(), qs[sb].groups[gi].slop.begin(), qs[sb].groups[gi].slop.end());
  }
  parallel_slabs(q_slabs, [&](uint32_t sb) {
    for (int gi = 0; gi < kNGroups; ++gi) {
      const Group &src = qs[sb].groups[gi];
      Group &g = b.groups[gi];
      const size_t at = g_base[gi][sb], n = src.queries.size();
      for (size_t i = 0; i < n; ++i) {
        g.queries[at + i] = src.queries[i];
        if (g.queries[at + i].thr_index != 0xFFFFFFFFu) g.queries[at + i].thr_index += thr_base[sb];
      }
      if (n) {
        memcpy(g.tile_cost.data() + at, src.tile_cost.data(), n * sizeof(uint32_t));
        memcpy(g.out_index.data() + at, src.out_index.data(), n * sizeof(uint32_t));
      }
    }
  });
  return TQ_OK;
}

// Every query into its launch group (plan_query), serially or in slabs.
int route_queries(Batch &b) {
  PlanScratch &ps = *b.ps;
  static const uint32_t kDenseRatioEnv = tune_u32("TQ_XU_RATIO", 0xFFFFFFFFu);  // (experiments: overrides the option)
  static const uint32_t kDenseMinEnv = tune_u32("TQ_XU_MIN_QUERIES", 0xFFFFFFFFu);
  b.dense_ratio = kDenseRatioEnv != 0xFFFFFFFFu ? kDenseRatioEnv : (uint32_t)b.s->opt.xunion_ratio;
  b.dense_min_queries = std::max<uint32_t>(1u, kDenseMinEnv != 0xFFFFFFFFu ? kDenseMinEnv : (uint32_t)b.s->opt.xunion_min_queries);
  b.groups = ps.groups;
  for (int gi = 0; gi < kNGroups; ++gi) {
    b.groups[gi].reset();
    b.groups[gi].mode = kGroupTraits[gi].mode;
  }
  ps.xrow_term.clear();
  ps.xrow_of.clear();
  ps.xcache = 0xFFFFFFFFu;
  b.t_route = Clock::now();  // (after validation of the context, the cache table and the pre-pass)
  static const uint32_t kQuerySlabMin = tune_u32("TQ_PLAN_QUERY_PAR_MIN", 4096);
  const uint32_t q_slabs = (!b.exhaustive && b.n_queries >= kQuerySlabMin) ? std::min<uint32_t>(plan_threads(), 8u) : 1u;
  if (q_slabs > 1) {
    const int rc = route_in_slabs(b, q_slabs);
    if (rc != TQ_OK) return rc;
  } else {
    for (uint32_t qi = 0; qi < b.n_queries; ++qi) {
      const int rc = plan_query(b, qi, b.groups, b.t);
      if (rc != TQ_OK) return rc;
    }
  }
  b.t_routed = Clock::now();
  // too few queries to pay for the tile rows: they keep the window kernel
  Group &d = b.groups[kGXUnion], &o = b.groups[kGUnion];
  if (!d.queries.empty() && d.queries.size() < b.dense_min_queries) {
    o.queries.append(d.queries.begin(), d.queries.end());
    o.tile_cost.insert(o.tile_cost.end(), d.tile_cost.begin(), d.tile_cost.end());
    o.out_index.insert(o.out_index.end(), d.out_index.begin(), d.out_index.end());
    o.max_k = std::max(o.max_k, d.max_k);
    d.reset();
    d.mode = kGroupTraits[kGXUnion].mode;
  }
  return TQ_OK;
}

// The wavefronts a shared-intersection launch keeps resident: its grid before the cap by the task count.
uint32_t ashare_resident(int cus) {
  static const uint32_t kAGridMul = tune_u32("TQ_AS_GRID_MUL", 0);
  return (uint32_t)std::max(1, cus) * (kAGridMul ? kAGridMul : tqk_ashare_waves_per_cu());
}

// Tiles -> chunks / tasks -> partial or result lists per group, in one buffer; `replan` if a shared launch is over budget.
int plan_group_tasks(Batch &b) {
  PlanScratch &ps = *b.ps;
  (void)hipDeviceGetAttribute(&b.cus, hipDeviceAttributeMultiprocessorCount, b.s->device);
  // (the intersections' one-dispatch rule counts on the launch's resident wavefronts: next to another group's kernels —
  // launch_groups runs them side by side — they are not its own, and the mixed stream measured 8 % slower with one dispatch)
  const bool alone = std::count_if(b.groups, b.groups + kNGroups, [](const Group &g) { return !g.queries.empty(); }) == 1;
  for (int gi = 0; gi < kNGroups; ++gi) {
    Group &g = b.groups[gi];
    if (g.queries.empty()) continue;
    if (gi == kGTree || gi == kGSlop) {  // one partial list per (query, tile of bitmap words); no chunk tables
      const uint32_t tiles = tqk_tree_tiles((b.s->max_doc + 31u) / 32u);
      g.kpl = kpl_for(g.max_k);
      for (TqdQuery &dq : g.queries) dq.n_parts = tiles;
      g.n_chunks = g.total_tiles = (uint32_t)g.queries.size() * tiles;
      continue;
    }
    if (gi == kGAll) {  // one partial list per (query, scanned tile): route_all set n_parts
      g.kpl = kpl_for(g.max_k);
      for (const TqdQuery &dq : g.queries) g.total_tiles += dq.n_parts;
      g.n_chunks = g.total_tiles;
      continue;
    }
    const int rc = gi == kGUShare   ? build_share_plan(b.s, g, ps)
                   : gi == kGAShare ? build_ashare_plan(b.s, g, ps, false, alone ? ashare_resident(b.cus) : 0u)
                   : gi == kGBShare ? build_ashare_plan(b.s, g, ps, true)
                   : gi == kGXUnion ? build_dense_plan(b.s, g, ps, (uint32_t)std::max(1, b.cus))
                                    : build_group_chunks(g, b.or_windows && gi != kGBool, ps, gi == kGBool);
    // (the same batch through the per-query kernels: nothing has been enqueued yet)
    if (rc == TQ_ERR_UNSUPPORTED && (gi == kGAShare || gi == kGBShare) && ps.ap[gi == kGBShare ? 1 : 0].over_budget) {
      (gi == kGBShare ? b.co.no_bshare : b.co.no_ashare) = true;
      b.replan = true;
    }
    if (rc != TQ_OK) return rc;
  }
  // partial lists of all groups share one buffer; its stride is per group (kpl*64 keys)
  for (int gi = 0; gi < kNGroups; ++gi) {
    Group &g = b.groups[gi];
    b.part_off_bytes[gi] = b.partial_bytes;
    if (kGroupTraits[gi].result_lists) {  // result lists: part_start / n_parts count 8-byte entries (build_share_plan)
      if (!g.queries.empty())  // (list_entries: the last query of a group may read an earlier query's list)
        b.partial_bytes += std::max<size_t>((size_t)g.list_entries, (size_t)g.queries.back().part_start + g.queries.back().n_parts) * sizeof(uint64_t);
      continue;
    }
    uint32_t parts = 0;
    for (TqdQuery &dq : g.queries) {
      dq.part_start = parts;
      parts += dq.n_parts;
    }
    b.partial_bytes += (size_t)parts * (size_t)g.kpl * 64u * sizeof(uint64_t);
  }
  Group &tree = b.groups[kGTree];
  for (size_t i = 0; i < tree.tree.size(); ++i) tree.tree[i].part_start = tree.queries[i].part_start;
  Group &all = b.groups[kGAll];
  for (size_t i = 0; i < all.all.size(); ++i) all.all[i].part_start = all.queries[i].part_start;
  Group &slop = b.groups[kGSlop];
  for (size_t i = 0; i < slop.slop.size(); ++i) slop.slop[i].part_start = slop.queries[i].part_start;
  return TQ_OK;
}

// Everything before the first enqueue: term records, probe tables, routing, the groups' tasks.
int plan_batch(Batch &b) {
  b.t0 = Clock::now();
  b.exhaustive = b.co.exhaustive;
  int rc = sync_term_records(b);
  if (rc != TQ_OK) return rc;
  look_at_queries(b);
  b.or_windows = b.s->opt.or_windows < 0 ? b.exhaustive : b.s->opt.or_windows != 0;
  if ((rc = build_flat_probe_tables(b)) != TQ_OK || (rc = build_tree_probe_tables(b)) != TQ_OK || (rc = build_all_probe_tables(b)) != TQ_OK) return rc;
  count_leaders(b);
  build_leader_norms(b);
  if ((rc = route_queries(b)) != TQ_OK) return rc;
  return plan_group_tasks(b);
}

// The staging blob's layout — [caches][per group: queries | tile_starts | out_index | chunks | sinks | the tables of
// the shared, doc-major and tree groups][new term records] — and the device scratch for the lists and match counts.
int lay_out_stage(Batch &b) {
  if (!b.sc->ev_last) HIP_TRY(hipEventCreateWithFlags(&b.sc->ev_last, hipEventDisableTiming));
  int rc = b.sc->partials.ensure(b.partial_bytes + 256);
  if (rc == TQ_OK) rc = b.s->d_qmatches.ensure((size_t)b.n_queries * sizeof(uint32_t));
  if (rc != TQ_OK) return rc;
  const PlanScratch &ps = *b.ps;
  b.copies.reserve(8 * kNGroups + b.caches.size());
  auto put = [&](size_t align, const void *src, size_t bytes) {
    b.stage = (b.stage + align - 1) & ~(align - 1);
    if (bytes && src) b.copies.push_back({b.stage, src, bytes});
    b.stage += bytes;
    return b.stage - bytes;
  };
  for (const float *c : b.caches) put(1, c, 256 * sizeof(float));
  for (int gi = 0; gi < kNGroups; ++gi) {
    Group &g = b.groups[gi];
    if (g.queries.empty()) continue;
    if (gi == kGAShare) {  // compact records + the full records of the queries with three and more lists: built by fill_stage
      g.o_queries = put(16, nullptr, g.queries.size() * sizeof(TqdAQuery));
      g.o_xqueries = put(16, nullptr, (size_t)b.t.n_ashare_ext * sizeof(TqdQuery));
    } else {
      g.o_queries = put(16, g.queries.data(), g.queries.size() * sizeof(TqdQuery));
    }
    g.o_tiles = put(16, g.tile_starts.data(), g.tile_starts.size() * sizeof(uint32_t));
    g.o_outidx = put(16, g.out_index.data(), g.out_index.size() * sizeof(uint32_t));
    g.o_chunks = put(16, g.chunk_recs.data(), g.chunk_recs.size() * sizeof(uint4));
    g.o_sinks = put(16, nullptr, sizeof(TqkSinks));  // (filled by fill_stage)
    if (gi == kGUShare) {
      g.o_leads = put(64, ps.leads.data(), ps.leads.size() * sizeof(TqdLead));
      g.o_tasks = put(16, ps.tasks.data(), ps.tasks.size() * sizeof(uint4));
    } else if (gi == kGAShare || gi == kGBShare) {
      const PlanScratch::ASharePlan &A = ps.ap[gi == kGBShare ? 1 : 0];
      g.o_leads = put(64, A.aleads.data(), A.aleads.size() * sizeof(TqdALead));
      g.o_tasks = put(16, A.atasks.data(), A.atasks.size() * sizeof(uint4));
      g.o_lists = put(16, A.alists.data(), gi == kGBShare ? A.alists.size() * sizeof(uint2) : 0);
    } else if (gi == kGTree) {  // (o_leads: the tree descriptors)
      g.o_leads = put(64, g.tree.data(), g.tree.size() * sizeof(TqdTreeQuery));
    } else if (gi == kGAll) {  // (o_leads: the ALL-BASED descriptors)
      g.o_leads = put(64, g.all.data(), g.all.size() * sizeof(TqdAllQuery));
    } else if (gi == kGSlop) {  // (o_leads: the sloppy phrases' descriptors)
      g.o_leads = put(64, g.slop.data(), g.slop.size() * sizeof(TqdSlopQuery));
    } else if (gi == kGXUnion) {  // (o_leads: the rows, o_tasks: the queries)
      g.o_leads = put(64, ps.xrows.data(), ps.xrows.size() * sizeof(TqkDenseRow));
      g.o_tasks = put(16, ps.xqueries.data(), ps.xqueries.size() * sizeof(TqkDenseQuery));
    }
  }
  b.o_terms = put(16, b.s->h_dterms.data() + b.terms_from, (b.terms_to - b.terms_from) * sizeof(TqdTerm));
  b.t_laid = Clock::now();
  return TQ_OK;
}

// The staging blob filled in pinned host memory (the buffer the previous batch's copy has left).
int fill_stage(Batch &b) {
  if (b.s->stage_in_flight) {  // (the pinned staging buffer is reused: the previous batch's copy must have left it)
    HIP_TRY(hipEventSynchronize(b.s->ev_stage_done));
    b.s->stage_in_flight = false;
  }
  b.t_waited = Clock::now();  // time spent waiting for the GPU is not planning time
  b.bx = (int)(b.s->batches_enqueued & 1u);
  // (both buffers grow with the first batch that needs it: a growth is a hipFree, i.e. a device-wide
  // synchronisation, and must not wait for the second batch of a new workload)
  int rc = b.s->h_stage.ensure(b.stage);
  if (rc == TQ_OK) rc = b.s->d_stage.ensure(b.stage);
  if (rc == TQ_OK) rc = b.s->d_stage_alt.ensure(b.stage);
  if (rc != TQ_OK) return rc;
  b.ds = (const uint8_t *)(b.bx ? b.s->d_stage_alt : b.s->d_stage).p;
  uint8_t *hs = (uint8_t *)b.s->h_stage.p;
  // the big tables (descriptors, chunk records: megabytes per 10 000-query batch) are copied by the planner's
  // threads, a quarter each
  for (const Batch::Copy &c : b.copies) {
    const uint32_t parts = c.bytes >= (1u << 20) ? std::min<uint32_t>(plan_threads(), 4u) : 1u;
    parallel_slabs(parts, [&](uint32_t pi) {
      const size_t x = (c.bytes * pi / parts) & ~(size_t)63, y = pi + 1 == parts ? c.bytes : (c.bytes * (pi + 1) / parts) & ~(size_t)63;
      memcpy(hs + c.off + x, (const uint8_t *)c.src + x, y - x);
    });
  }
  {  // the shared intersections' queries as the launch and its merge read them (TqdAQuery)
    const Group &g = b.groups[kGAShare];
    TqdAQuery *aq = (TqdAQuery *)(hs + g.o_queries);
    TqdQuery *xq = (TqdQuery *)(hs + g.o_xqueries);
    uint32_t n_ext = 0;
    for (size_t q = 0; q < g.queries.size(); ++q) {
      const TqdQuery &dq = g.queries[q];
      TqdAQuery r{};
      r.part_start = dq.part_start;
      r.chunk_first = dq.chunk_first;
      r.k = dq.k;
      r.term1 = dq.term[1];
      r.n_terms = dq.n_terms;
      r.ext = 0xFFFFFFFFu;
      if (dq.n_terms > 2u) {
        if (n_ext == b.t.n_ashare_ext) return fail(TQ_ERR_INVALID, "shared intersections: more queries of three and more lists than were routed");
        r.ext = n_ext;
        xq[n_ext++] = dq;
      }
      aq[q] = r;
    }
  }
  for (int gi = 0; gi < kNGroups; ++gi) {
    const Group &g = b.groups[gi];
    if (g.queries.empty()) continue;
    TqkSinks sk{};
    sk.partials = (uint64_t *)((uint8_t *)b.sc->partials.p + b.part_off_bytes[gi]);
    sk.match_counter = b.s->d_match_counter;
    sk.query_matches = (uint32_t *)b.s->d_qmatches.p;
    sk.out_index = (const uint32_t *)(b.ds + g.o_outidx);
    memcpy(hs + g.o_sinks, &sk, sizeof sk);
  }
  b.t_filled = Clock::now();
  return TQ_OK;
}

// This batch after the previous one on the segment and after whichever batch used the device's scratch last.
int order_batch(Batch &b) {
  b.slot = (int)(b.s->batches_timed % tq_segment::kTimingRing);
  // the scratch below is shared with the previous batch: wait for it if it ran on another stream
  const int rc = order_after_last_batch(b.s, b.st);
  if (rc != TQ_OK) return rc;
  // ... and the device's shared scratch with whichever segment's batch used it last
  if (b.sc->in_flight && b.sc->last_stream != b.st) HIP_TRY(hipStreamWaitEvent(b.st, b.sc->ev_last, 0));
  if (b.s->opt.timing) HIP_TRY(hipEventRecord(b.s->ev_t0[b.slot], b.st));
  return TQ_OK;
}

// The leaders' doc-matrix words in posting order this batch planned with (build_leader_norms): filled on the batch's
// stream, behind every earlier batch of the segment (a refill rewrites a table those may read) and ahead of its kernels.
// (a plan that is dropped before its tables were filled — a replan, an error on the way — leaves them marked stale)
void drop_leader_mats(Batch &b) {
  for (uint32_t h : b.lmat_fill) b.s->terms[h].lmat_epoch = 0;
  b.lmat_fill.clear();
}
int fill_leader_mats(Batch &b) {
  for (uint32_t h : b.lmat_fill) {
    const hipError_t e = fill_lmat(b.s, h, b.st);
    if (e != hipSuccess) {
      drop_leader_mats(b);
      return fail(TQ_ERR_HIP, "leader doc-matrix words: %s", hipGetErrorString(e));
    }
  }
  b.lmat_fill.clear();
  return TQ_OK;
}

// The staging blob up on the copy stream, the new term records into the table's tail on the batch's stream.
int enqueue_copy(Batch &b) {
  // buffer bx was last read by the batch before the previous one: the copy waits for that
  // batch's end (recorded on its stream), the kernels below wait for the copy
  if (b.s->buf_used[b.bx]) HIP_TRY(hipStreamWaitEvent(b.s->copy_stream, b.s->ev_buf_free[b.bx], 0));
  HIP_TRY(hipMemcpyAsync((void *)b.ds, b.s->h_stage.p, b.stage, hipMemcpyHostToDevice, b.s->copy_stream));
  HIP_TRY(hipEventRecord(b.s->ev_stage_done, b.s->copy_stream));
  HIP_TRY(hipEventRecord(b.s->ev_copy_done[b.bx], b.s->copy_stream));
  HIP_TRY(hipStreamWaitEvent(b.st, b.s->ev_copy_done[b.bx], 0));
  b.s->stage_in_flight = true;
  if (b.terms_to > b.terms_from) {  // the new term records: staging blob -> the table's tail, in stream order before the kernels
    HIP_TRY(hipMemcpyAsync(b.s->d_terms + b.terms_from, b.ds + b.o_terms, (b.terms_to - b.terms_from) * sizeof(TqdTerm),
                           hipMemcpyDeviceToDevice, b.st));
    b.s->d_terms_dirty = false;
    b.s->d_terms_dirty_from = ~(size_t)0;
    b.s->d_terms_synced = b.terms_to;
  }
  return TQ_OK;
}

// A result-list group's words (thr_val | list_count per query, task counters) and its grid's staging lists (the
// doc-major group is unpruned, the shared-union group pruned: they never meet in one batch and share both).
DevBuf &list_words(tq_segment *s, int gi) {
  return gi == kGAShare ? s->d_ashare_words : gi == kGBShare ? s->d_bshare_words : s->d_share_words;
}
DevBuf &list_stage(DeviceScratch &sc, int gi) {
  return gi == kGAShare ? sc.ashare_stage : gi == kGBShare ? sc.bshare_stage : sc.share_stage;
}

// Every buffer the batch zeroes, cleared by one launch; the result-list groups' grids, words and staging lists.
int zero_batch_buffers(Batch &b) {
  TqkZeroParams zp{};
  auto zero_later = [&](void *ptr, size_t bytes) -> int {
    if (!bytes) return TQ_OK;
    if (zp.n == (uint32_t)TQK_ZERO_MAX || (bytes & 3u) || ((uintptr_t)ptr & 3u) || bytes > 0xFFFFFFFFull * 4u) {
      HIP_TRY(hipMemsetAsync(ptr, 0, bytes, b.st));  // (never taken today: at most six aligned buffers)
      return TQ_OK;
    }
    zp.ptr[zp.n] = (uint32_t *)ptr;
    zp.words[zp.n++] = (uint32_t)(bytes >> 2);
    return TQ_OK;
  };
  int rc = zero_later(b.s->d_match_counter, sizeof(unsigned long long));
  if (rc == TQ_OK) rc = zero_later(b.s->d_qmatches.p, (size_t)b.n_queries * sizeof(uint32_t));
  if (rc != TQ_OK) return rc;
  b.s->last_batch_queries = b.n_queries;
  b.s->last_batch_slop = !b.groups[kGSlop].queries.empty();
  b.s->slop_over_words = b.n_queries;
  if (b.s->last_batch_slop) {  // the sloppy phrases' overflow words, one per query of the batch
    rc = b.s->d_slop_over.ensure((size_t)b.n_queries * sizeof(uint32_t));
    if (rc == TQ_OK) rc = zero_later(b.s->d_slop_over.p, (size_t)b.n_queries * sizeof(uint32_t));
    if (rc != TQ_OK) return rc;
  }
  if (b.t.n_thr_rows) {
    const size_t thr_bytes = (size_t)b.t.n_thr_rows * TQD_THR_SLOTS * sizeof(uint32_t);
    rc = b.s->d_thr.ensure(thr_bytes);
    if (rc == TQ_OK) rc = zero_later(b.s->d_thr.p, thr_bytes);
    if (rc != TQ_OK) return rc;
  }
  static const uint32_t kGridMul = std::max<uint32_t>(1u, tune_u32("TQ_US_GRID_MUL", 16));
  static const uint32_t kAGridMul = tune_u32("TQ_AS_GRID_MUL", 0);
  const uint64_t cus = (uint64_t)std::max(1, b.cus);
  for (int gi : {kGXUnion, kGUShare, kGAShare, kGBShare}) {
    const Group &g = b.groups[gi];
    const size_t n = g.queries.size();
    if (!n) continue;
    const uint32_t per_cu = gi == kGXUnion ? 0u : gi == kGUShare ? kGridMul : kAGridMul ? kAGridMul
                            : gi == kGBShare ? tqk_bshare_waves_per_cu() : tqk_ashare_waves_per_cu();
    b.grid[gi] = gi == kGXUnion ? b.ps->xgrid : (uint32_t)std::min<uint64_t>(g.n_chunks, cus * per_cu);
    const size_t stage_lists = (size_t)b.grid[gi] * (gi == kGXUnion ? n : gi == kGUShare ? TQD_US_GROUP : TQD_AS_GROUP);
    const size_t words = 2 * n + 16;  // (+ up to 16 task counters: one per launch)
    rc = list_words(b.s, gi).ensure(words * sizeof(uint32_t));
    if (rc == TQ_OK) rc = list_stage(*b.sc, gi).ensure(stage_lists * tqk_share_capl(g.kpl) * sizeof(uint64_t));
    if (rc == TQ_OK) rc = zero_later(list_words(b.s, gi).p, words * sizeof(uint32_t));
    if (rc != TQ_OK) return rc;
  }
  return launched(tqk_launch_zero(zp, b.st), "zero");
}

// The fields the per-query, shared-union and shared-intersection launches have in common.
template <typename P>
void common_params(P &p, const Batch &b, const Group &g) {
  p.seg = b.s->dseg;
  p.terms = b.s->d_terms;
  p.queries = (const TqdQuery *)(b.ds + g.o_queries);
  p.caches = (const float *)(b.ds + b.o_caches);
  p.sinks = (const TqkSinks *)(b.ds + g.o_sinks);
  p.thr_slots = (uint32_t *)b.s->d_thr.p;
  p.debug = b.s->opt.debug >= 0 ? (uint32_t)b.s->opt.debug : knobs().debug;  // (option "debug": work counters of one batch, bench.py)
  p.bound_slack = b.co.bound_slack;
}

// A shared-intersection launch: the warm-up tasks, then the rest (stream order = the barrier between them) — or, where
// build_ashare_plan put the independent main tasks behind the warm-up tasks (ASharePlan::a_inline), all of them at once.
int launch_ashare(const Batch &b, int gi, hipStream_t gst) {
  const Group &g = b.groups[gi];
  const int ai = gi == kGBShare ? 1 : 0;
  const size_t n_a = g.queries.size();
  TqkAShareParams ap{};
  common_params(ap, b, g);
  if (gi == kGAShare) {
    ap.queries = nullptr;
    ap.aqueries = (const TqdAQuery *)(b.ds + g.o_queries);
    ap.xqueries = (const TqdQuery *)(b.ds + g.o_xqueries);
  }
  ap.leads = (const TqdALead *)(b.ds + g.o_leads);
  ap.tasks = (const uint4 *)(b.ds + g.o_tasks);
  ap.qlists = (const uint2 *)(b.ds + g.o_lists);
  ap.thr_val = (uint32_t *)list_words(b.s, gi).p;
  ap.list_count = ap.thr_val + n_a;
  ap.table_base = (const uint8_t *)b.ps->share_table_base;
  ap.stage = (uint64_t *)list_stage(*b.sc, gi).p;
  ap.lists = (uint64_t *)((uint8_t *)b.sc->partials.p + b.part_off_bytes[gi]);
  ap.n_queries = (uint32_t)n_a;
  ap.boolean = (uint32_t)ai;
  ap.rdir_lists = ai && b.ps->ap[ai].any_rdir ? 1u : 0u;
  // TQ_AS_BOUND (A/B of the bound on the non-leader list of an intersection; every setting is exact):
  // bit 0 the block pre-filter takes list 1's range maxima over the leader block's doc span, bit 1 the
  // gather cut of a block comes from that pre-filter, bit 2 the per-(doc, lead) test reads the doc's own
  // range (measured slower: two more dependent byte gathers per (block, lead) pair cost more than the 7 % of
  // scoring-stage candidates they remove); 0 = round 4: list 1 is bounded by its weight.  Default 3.
  static const uint32_t kBoundMode = tune_u32("TQ_AS_BOUND", 3);
  ap.bound_mode = kBoundMode;
  ap.n_queues = 1;
  const uint32_t bounds[3] = {0u, b.ps->ap[ai].a_inline ? g.n_chunks : b.ps->ap[ai].a_warm_tasks, g.n_chunks};
  for (int ph = 0; ph < 2; ++ph) {
    ap.task_begin = bounds[ph];
    ap.n_tasks = bounds[ph + 1];
    if (ap.n_tasks <= ap.task_begin) continue;
    ap.task_counter = ap.thr_val + 2 * n_a + 8 * ph;
    ap.grid = std::min<uint32_t>(b.grid[gi], ap.n_tasks - ap.task_begin);
    const int rc = launched(tqk_launch_ashare(ap, g.kpl, gst), "shared-intersection");
    if (rc != TQ_OK) return rc;
  }
  return TQ_OK;
}

// The shared-union launch: one launch per list position (stream order = the barrier between positions).
int launch_ushare(const Batch &b, hipStream_t gst) {
  const Group &g = b.groups[kGUShare];
  const size_t n_share = g.queries.size();
  TqkShareParams sp{};
  common_params(sp, b, g);
  sp.leads = (const TqdLead *)(b.ds + g.o_leads);
  sp.tasks = (const uint4 *)(b.ds + g.o_tasks);
  sp.thr_val = (uint32_t *)b.s->d_share_words.p;
  sp.list_count = sp.thr_val + n_share;
  uint32_t *const counters = sp.thr_val + 2 * n_share;  // one task counter per launch
  sp.stage = (uint64_t *)b.sc->share_stage.p;
  sp.lists = (uint64_t *)((uint8_t *)b.sc->partials.p + b.part_off_bytes[kGUShare]);
  sp.n_queries = (uint32_t)n_share;
  sp.table_base = (const uint8_t *)b.ps->share_table_base;
  static const uint32_t kPhases = tune_u32("TQ_US_PHASES", 0);
  for (uint32_t ph = 0; ph < TQD_US_MAX_TERMS; ++ph) {
    sp.task_begin = b.ps->share_phase_first[ph];
    sp.n_tasks = b.ps->share_phase_first[ph + 1];
    if (!kPhases) {  // (experiments) one launch, tasks still in position order
      if (ph) break;
      sp.n_tasks = g.n_chunks;
    }
    if (sp.n_tasks <= sp.task_begin) continue;
    sp.task_counter = counters + ph;
    sp.grid = std::min<uint32_t>(b.grid[kGUShare], sp.n_tasks - sp.task_begin);
    const int rc = launched(tqk_launch_share(sp, g.kpl, gst), "shared-union");
    if (rc != TQ_OK) return rc;
  }
  return TQ_OK;
}

// The nested boolean queries over bitmap words.
int launch_tree(const Batch &b, hipStream_t gst) {
  const Group &g = b.groups[kGTree];
  TqkTreeParams tp{};
  tp.seg = b.s->dseg;
  tp.terms = b.s->d_terms;
  tp.queries = (const TqdTreeQuery *)(b.ds + g.o_leads);
  tp.caches = (const float *)(b.ds + b.o_caches);
  tp.sinks = (const TqkSinks *)(b.ds + g.o_sinks);
  tp.table_base = (const uint8_t *)b.s->share_table_lo;
  tp.n_queries = (uint32_t)g.queries.size();
  tp.n_words = (b.s->max_doc + 31u) / 32u;
  bool any_field = false;  // some list of the launch belongs to a non-primary field: per-list norms (tq_fields.cpp)
  for (const TqdTreeQuery &tq : g.tree) {
    tp.any_phrase |= tq.has_phrase;
    for (uint32_t t = 0; b.s->n_field_terms && t < tq.n_terms; ++t) any_field = any_field || (tq.atom_end[t] >> 4) != 0u;
  }
  if (any_field) {
    TqkTreeFieldsParams fp{};
    fp.base = tp;
    fp.fn[0] = b.s->d_fn;
    for (uint32_t f = 1; f < TQK_MAX_FIELDS; ++f) fp.fn[f] = b.s->d_fn_field[f];
    return launched(tqk_launch_tree_fields(fp, g.kpl, gst), "nested boolean (multi-field)");
  }
  return launched(tqk_launch_tree(tp, g.kpl, gst), "nested boolean");
}

// The ALL-BASED queries over bitmap words.
int launch_all(const Batch &b, hipStream_t gst) {
  const Group &g = b.groups[kGAll];
  TqkAllParams ap{};
  ap.seg = b.s->dseg;
  ap.terms = b.s->d_terms;
  ap.queries = (const TqdAllQuery *)(b.ds + g.o_leads);
  ap.caches = (const float *)(b.ds + b.o_caches);
  ap.sinks = (const TqkSinks *)(b.ds + g.o_sinks);
  ap.table_base = (const uint8_t *)b.s->share_table_lo;
  ap.n_queries = (uint32_t)g.queries.size();
  ap.n_words = (b.s->max_doc + 31u) / 32u;
  for (const TqdAllQuery &aq : g.all) ap.max_tiles = std::max(ap.max_tiles, aq.n_tiles);
  return launched(tqk_launch_all(ap, g.kpl, gst), "match-all");
}

// The sloppy phrases over bitmap words: one launch per instantiation the group needs.
int launch_slop(const Batch &b, hipStream_t gst) {
  const Group &g = b.groups[kGSlop];
  TqkPhraseSlopParams sp{};
  sp.seg = b.s->dseg;
  sp.terms = b.s->d_terms;
  sp.queries = (const TqdSlopQuery *)(b.ds + g.o_leads);
  sp.caches = (const float *)(b.ds + b.o_caches);
  sp.sinks = (const TqkSinks *)(b.ds + g.o_sinks);
  sp.table_base = (const uint8_t *)b.s->share_table_lo;
  sp.overflow = (uint32_t *)b.s->d_slop_over.p;
  sp.n_queries = (uint32_t)g.queries.size();
  sp.n_words = (b.s->max_doc + 31u) / 32u;
  for (const TqdSlopQuery &sq : g.slop) (sq.n_terms > 2u ? sp.any_carry : sp.any_pair) = 1u;
  return launched(tqk_launch_phrase_slop(sp, g.kpl, gst), "sloppy phrase");
}

// The doc-major union launch.
int launch_xunion(const Batch &b, hipStream_t gst) {
  const PlanScratch &ps = *b.ps;
  const Group &g = b.groups[kGXUnion];
  const size_t n_dense = g.queries.size();
  TqkDenseParams dp{};
  dp.seg = b.s->dseg;
  dp.terms = b.s->d_terms;
  dp.rows = (const TqkDenseRow *)(b.ds + g.o_leads);
  dp.queries = (const TqkDenseQuery *)(b.ds + g.o_tasks);
  dp.cache = (const float *)(b.ds + b.o_caches) + (size_t)ps.xcache * 256u;
  dp.sinks = (const TqkSinks *)(b.ds + g.o_sinks);
  dp.thr_slots = (uint32_t *)b.s->d_thr.p;
  dp.thr_val = (uint32_t *)b.s->d_share_words.p;
  dp.list_count = dp.thr_val + n_dense;
  dp.task_counter = dp.thr_val + 2 * n_dense;
  dp.stage = (uint64_t *)b.sc->share_stage.p;
  dp.lists = (uint64_t *)((uint8_t *)b.sc->partials.p + b.part_off_bytes[kGXUnion]);
  dp.n_rows = (uint32_t)ps.xrows.size();
  dp.n_bitmap_rows = ps.x_bitmap_rows;
  dp.n_queries = (uint32_t)n_dense;
  dp.max_terms = ps.x_max_terms;
  dp.n_tasks = g.n_chunks;
  dp.tiles_per_task = ps.x_tiles_per_task;
  dp.list_stride = ps.x_list_stride;
  dp.grid = b.grid[kGXUnion];
  dp.debug = knobs().debug;
  return launched(tqk_launch_xunion(dp, g.kpl, gst), "doc-major union");
}

// The per-query scan kernels (and_kernel, union / or-window kernels, phrase kernels).
int launch_scan(const Batch &b, int gi, hipStream_t gst) {
  const Group &g = b.groups[gi];
  TqkScanParams p{};
  common_params(p, b, g);
  if (!b.s->opt.use_dense) p.seg.docmat = nullptr, p.seg.doccls = nullptr;
  p.tile_starts = (const uint32_t *)(b.ds + g.o_tiles);
  p.n_queries = (uint32_t)g.queries.size();
  p.total_tiles = g.total_tiles;
  p.chunk_recs = (const uint4 *)(b.ds + g.o_chunks);
  p.n_chunks = g.n_chunks;
  p.exhaustive = (uint32_t)b.exhaustive;
  p.use_dense = (uint32_t)b.s->opt.use_dense;
  p.all_dense = (gi == kGAndDense || (gi == kGPhrase && b.t.phrase_all_dense)) ? 1u : 0u;
  p.or_windows = gi == kGPhSweep ? 2u : ((b.or_windows && gi != kGBool) ? 1u : 0u);  // (2 = phrase sweep)
  p.boolean = gi == kGBool ? 1u : 0u;
  p.small_k = g.max_k <= 16u ? 1u : 0u;
  p.max_terms = 0;
  for (const TqdQuery &dq : g.queries) p.max_terms = std::max(p.max_terms, dq.n_terms);
  const bool dpp = b.s->opt.use_dpp != 0;
  return launched(g.mode == TQ_MODE_AND  ? tqk_launch_and(p, g.kpl, dpp, gst)
                  : g.mode == TQ_MODE_OR ? tqk_launch_or(p, g.kpl, dpp, gst)
                                         : tqk_launch_phrase(p, g.kpl, dpp, gst),
                  "scan kernel");
}

// The scan kernels of every group.  They are independent: all but the main group's run on the segment's side stream,
// forked from and joined back into the batch's stream with events, so that a small group (e.g. the AND queries over
// sparse lists) fills the gaps of the big one instead of adding its own ramp-up and tail.
int launch_groups(Batch &b) {
  const Group *groups = b.groups;
  if (b.s->opt.timing) HIP_TRY(hipEventRecord(b.s->ev_k0[b.slot], b.st));
  const bool fork = std::count_if(groups, groups + kNGroups, [](const Group &g) { return !g.queries.empty(); }) > 1;
  if (fork) {
    HIP_TRY(hipEventRecord(b.s->ev_fork, b.st));
    HIP_TRY(hipStreamWaitEvent(b.s->side_stream, b.s->ev_fork, 0));
  }
  // the group that keeps the caller's stream: the batch's intersections
  // (a batch without either: the phrase sweep, else the first group that has queries — two groups that both went to the
  // side stream ran one after the other: the few sparse-leader phrases of a phrase batch added their 0.26 ms)
  int main_group = -1;
  for (int gi : {kGAShare, kGAndDense, kGPhSweep})
    if (main_group < 0 && !groups[gi].queries.empty()) main_group = gi;
  for (int gi = 0; main_group < 0 && gi < kNGroups; ++gi)
    if (!groups[gi].queries.empty()) main_group = gi;
  // long serial chains first
  for (const int gi : {kGAnd, kGBool, kGBShare, kGUShare, kGXUnion, kGTree, kGSlop, kGAll, kGUnion, kGPhrase, kGPhSweep, kGAndDense, kGAShare}) {
    if (groups[gi].queries.empty()) continue;
    const hipStream_t gst = (fork && gi != main_group) ? b.s->side_stream : b.st;
    const int rc = gi == kGAShare || gi == kGBShare ? launch_ashare(b, gi, gst)
                   : gi == kGUShare                ? launch_ushare(b, gst)
                   : gi == kGTree                  ? launch_tree(b, gst)
                   : gi == kGAll                   ? launch_all(b, gst)
                   : gi == kGSlop                  ? launch_slop(b, gst)
                   : gi == kGXUnion                ? launch_xunion(b, gst)
                                                   : launch_scan(b, gi, gst);
    if (rc != TQ_OK) return rc;
  }
  if (fork) {
    HIP_TRY(hipEventRecord(b.s->ev_join, b.s->side_stream));
    HIP_TRY(hipStreamWaitEvent(b.st, b.s->ev_join, 0));
  }
  if (b.s->opt.timing) HIP_TRY(hipEventRecord(b.s->ev_k1[b.slot], b.st));
  return TQ_OK;
}

// Every group's partial / result lists -> the caller's top-k rows.
int launch_merges(const Batch &b) {
  for (int gi = 0; gi < kNGroups; ++gi) {
    const Group &g = b.groups[gi];
    if (g.queries.empty()) continue;
    TqkMergeParams m{};
    m.queries = (const TqdQuery *)(b.ds + g.o_queries);
    m.partials = (const uint64_t *)((const uint8_t *)b.sc->partials.p + b.part_off_bytes[gi]);
    m.out_index = (const uint32_t *)(b.ds + g.o_outidx);
    m.out_scores = b.out_scores;
    m.out_docs = b.out_docs;
    m.out_counts = b.out_counts;
    m.out_segment_ords = b.out_segment_ords;
    m.segment_ord = b.segment_ord;
    m.n_queries = (uint32_t)g.queries.size();
    m.out_stride = b.out_stride;
    if (!kGroupTraits[gi].result_lists) {
      // a query with hundreds of partial lists (a small batch cut into short tiles): its lists are reduced by up
      // to 32 wavefronts first — one wavefront walking 2 000 lists was most of a one-query call
      uint32_t max_parts = 0;
      for (const TqdQuery &dq : g.queries) max_parts = std::max(max_parts, dq.n_parts);
      if (max_parts >= TQK_MERGE_PRE_MIN && m.n_queries <= 4096u)
        m.pre_slices = std::min<uint32_t>(32u, std::max<uint32_t>(2u, (uint32_t)std::sqrt((double)max_parts)));
    }
    const int rc = launched(kGroupTraits[gi].result_lists
                                ? tqk_launch_merge_lists(m, (const uint32_t *)list_words(b.s, gi).p + g.queries.size(), g.kpl, gi == kGAShare, b.st)
                                : tqk_launch_merge(m, g.kpl, b.st),
                            "merge kernel");
    if (rc != TQ_OK) return rc;
  }
  // a host-output batch with sloppy phrases: their overflow words behind the rows, in stream order (the next batch zeroes them)
  if (b.s->last_batch_slop && b.co.h_slop_over)
    HIP_TRY(hipMemcpyAsync(b.co.h_slop_over, b.s->d_slop_over.p, (size_t)b.n_queries * sizeof(uint32_t), hipMemcpyDeviceToHost, b.st));
  return TQ_OK;
}

// The events behind the batch's last kernel, the batch's stats and kernel families, TQ_TRACE's line.
int finish_batch(const Batch &b) {
  DeviceScratch &sc = *b.sc;
  if (b.s->opt.timing) {
    HIP_TRY(hipEventRecord(b.s->ev_t1[b.slot], b.st));
    ++b.s->batches_timed;
  }
  HIP_TRY(hipEventRecord(b.s->ev_batch_done, b.st));
  HIP_TRY(hipEventRecord(sc.ev_last, b.st));
  sc.last_stream = b.st;
  sc.in_flight = true;
  HIP_TRY(hipEventRecord(b.s->ev_buf_free[b.bx], b.st));
  b.s->buf_used[b.bx] = true;
  ++b.s->batches_enqueued;
  b.s->last_stream = b.st;
  b.s->batch_in_flight = true;
  uint32_t kernel_mask = 0, tiles_total = 0, chunks_total = 0;
  if (b.s->opt.record_query_kernels) b.s->last_query_kernel.assign(b.n_queries, 0u);  // (tq_last_batch_query_kernels)
  for (int gi = 0; gi < kNGroups; ++gi) {
    const Group &g = b.groups[gi];
    if (g.queries.empty()) continue;
    const uint32_t bit = group_kernel_bit(gi, b.or_windows);
    kernel_mask |= bit;
    tiles_total += g.total_tiles;
    chunks_total += g.n_chunks;
    if (b.s->opt.record_query_kernels)
      for (uint32_t qi : g.out_index) b.s->last_query_kernel[qi] = bit;
  }
  static const bool trace = getenv("TQ_TRACE") != nullptr;
  if (trace) {
    const auto t_enqueued = Clock::now();
    auto us = [](auto x, auto y) { return (long)std::chrono::duration_cast<std::chrono::microseconds>(y - x).count(); };
    for (int gi = 0; gi < kNGroups; ++gi)
      if (!b.groups[gi].queries.empty())
        fprintf(stderr, "[tq] group %d: %zu queries, %u tasks\n", gi, b.groups[gi].queries.size(), b.groups[gi].n_chunks);
    fprintf(stderr, "[tq] plan %ld us (pre-pass %ld us, queries %ld us, chunks %ld us), wait for the staging buffer %ld us, stage fill %ld us, enqueue %ld us, stage bytes %zu\n",
            us(b.t0, b.t_laid), us(b.t0, b.t_route), us(b.t_route, b.t_routed), us(b.t_routed, b.t_laid), us(b.t_laid, b.t_waited),
            us(b.t_waited, b.t_filled), us(b.t_filled, t_enqueued), b.stage);
  }
  b.s->stats.algorithmic_bytes = b.t.algo_bytes;
  b.s->stats.tiles = tiles_total;
  b.s->stats.chunks = chunks_total;
  b.s->stats.matches = 0;
  b.s->stats.kernel_ms = 0;
  b.s->stats.total_ms = 0;
  b.s->stats.host_plan_ms = 0;
  b.s->stats.kernel_mask = kernel_mask;
  b.s->stats.unique_bytes = b.unique_bytes;
  b.s->stats_pending = true;
  b.s->stats_match_bytes = 1;
  b.s->stats_sorted = false;
  return TQ_OK;
}

// From the first enqueue on, work is in flight that reads the staging buffer: a failure must not let the next call
// overwrite it under kernels that were already launched (the events that order the buffers are only recorded at the
// end), so every error return first drains the streams.
struct DrainOnError {
  tq_segment *s;
  hipStream_t st;
  bool armed = true;
  ~DrainOnError() {
    if (!armed) return;
    if (s->copy_stream) (void)hipStreamSynchronize(s->copy_stream);
    if (s->side_stream) (void)hipStreamSynchronize(s->side_stream);
    (void)hipStreamSynchronize(st);
  }
};

// The one pre-pass over the caller's queries before anything is planned: AllQuery clauses (TQ_TERM_ALL) and term sets.
// All clauses: the normal form of tq_all.cpp decides each query — EMPTY and PLAIN ones are replaced by their stripped
// views (today's kernels see a query without All clauses, and a PLAIN query's rows are that query's, bit for bit),
// ALL-BASED ones stay as they are for route_all.
// Term sets (tq_termset.cpp; looked for only on a segment that has ever had one: s->n_set_slots): the reference runs a
// query through the generic, unpruned for_each_pruning_scorer as soon as one of its scorers is not a TermScorer
// (boolean_weight.rs:44-86, intersection.rs:39-55): here that is tree_kernel, whatever the query's mode.  Such a query is
// flagged (set_q[qi]: plan_query and the probe-table pass test the flag, no handle is looked at again) and counted; a
// TQ_MODE_AND / TQ_MODE_OR one gets its occurs on call scratch.  Refused: a set in a phrase or released (TQ_ERR_INVALID),
// inside a nested query, or as a Should clause of an ALL-BASED query (TQ_ERR_UNSUPPORTED: all_kernel takes sets as
// MustNot lists only).  A batch without an All clause or a set is not copied.
struct AllStrip {
  std::vector<tq_query> eff;
  std::deque<AllView> views;  // (a deque: the views' arrays stay where they are)
  std::deque<std::array<uint8_t, TQ_MAX_TERMS>> set_occurs;  // the occurs of TQ_MODE_AND / TQ_MODE_OR queries that name a set
  std::vector<uint8_t> set_q;  // per query: it names a term set and runs as a tree (empty: no query of the batch does)
  std::deque<TreeView> field_phrases;  // TQ_MODE_PHRASE queries of a non-primary field as one-atom trees
  std::deque<SlopView> slop_views;     // TQ_MODE_PHRASE queries with slop > 0 as one-atom trees in cost order (tq_phrase_slop.cpp)
  std::vector<uint32_t> slop_q;        // per query: its slop (empty: no query of the batch has one)
  uint32_t n_all_based = 0, n_set = 0;
};
int strip_all_clauses(const tq_segment *s, const tq_query *queries, uint32_t n_queries, AllStrip &st) {
  const bool sets = s->n_set_slots != 0;
  // Multi-field segments (tq_fields.cpp; looked for only while the segment holds a prepared term of a field != 0): a
  // query that names such a term scores per LIST norms — tree_fields_kernel, tq_tree_fields.hip, whatever its mode,
  // flagged in set_q like a query that names a set (the same route: occurs on call scratch, every list through a
  // bitmap, nothing pruned).  A TQ_MODE_PHRASE query becomes the tree "one Must clause holding one phrase atom".
  const bool fields = s->n_field_terms != 0;
  for (uint32_t qi = 0; qi < n_queries; ++qi) {
    if (queries[qi].slop) {  // a sloppy phrase: its own launch group (route_slop), planned from its view
      st.slop_views.emplace_back();
      const int vrc = slop_view(s, queries[qi], qi, "tq_search_batch", st.slop_views.back(), true);
      if (vrc != TQ_OK) return vrc;
      if (st.eff.empty()) st.eff.assign(queries, queries + n_queries);
      st.eff[qi] = st.slop_views.back().v.q;
      if (st.slop_q.empty()) st.slop_q.assign(n_queries, 0);
      st.slop_q[qi] = queries[qi].slop;
      continue;
    }
    bool names_set = false;
    if (sets) {
      const int src = check_set_query(s, queries[qi], qi, "tq_search_batch", &names_set);
      if (src != TQ_OK) return src;
    }
    bool names_field = false;
    if (fields && query_names_field(s, queries[qi])) {
      const int frc = check_field_query(s, queries[qi], qi, "tq_search_batch");
      if (frc != TQ_OK) return frc;
      names_field = true;
      if (queries[qi].mode == TQ_MODE_PHRASE) {
        const tq_query &pq = queries[qi];
        if (pq.n_terms < 2 || !pq.phrase_offsets || !pq.weights) return fail(TQ_ERR_INVALID, "query %u: a phrase needs >= 2 terms, offsets and a weight", qi);
        if (st.eff.empty()) st.eff.assign(queries, queries + n_queries);
        st.field_phrases.emplace_back();
        docset_tree_view(pq, st.field_phrases.back(), true);
        st.eff[qi] = st.field_phrases.back().q;
        if (st.set_q.empty()) st.set_q.assign(n_queries, 0);
        st.set_q[qi] = 1;
        ++st.n_set;
        continue;
      }
    }
    bool all_based = false;
    if (query_has_all(queries[qi])) {
      AllForm f;
      const char *why = "";
      const int rc = all_query_form(queries[qi], f, &why);
      if (rc != TQ_OK) return fail(rc, "query %u: %s", qi, why);
      if (f.boost_mixed)
        return fail(TQ_ERR_UNSUPPORTED, "query %u has a boosted match-all clause beside another scoring clause or a second match-all clause: its scores stay on the CPU", qi);
      all_based = f.kind == TQ_ALL_BASED;
      if (all_based) {
        ++st.n_all_based;
      } else {
        if (st.eff.empty()) st.eff.assign(queries, queries + n_queries);
        st.views.emplace_back();
        all_strip_view(queries[qi], f, st.views.back());
        st.eff[qi] = st.views.back().q;
      }
    }
    if (!names_set && !names_field) continue;
    const tq_query &q = st.eff.empty() ? queries[qi] : st.eff[qi];  // (what is left of it without its All clauses)
    if (all_based) {
      for (uint32_t i = 0; i < q.n_terms; ++i) {
        const bool must_not = q.mode == TQ_MODE_BOOL && q.occurs && q.occurs[i] == TQ_MUST_NOT;
        if (is_term_set(s, q.terms[i]) && !must_not)
          return fail(TQ_ERR_UNSUPPORTED, "tq_search_batch: query %u: a term set as a Should clause beside a match-all clause stays on the CPU (its counts and doc sets are taken)", qi);
        if (names_field && term_field_of(s, q.terms[i]) && !must_not)  // (all_kernel scores under field 0's norms)
          return fail(TQ_ERR_UNSUPPORTED, "tq_search_batch: query %u: a Should term of field %u (the scoring terms of a query whose match-all clauses make every doc a candidate are its Should terms) stays on the CPU (its counts and doc sets are taken)", qi, term_field_of(s, q.terms[i]));
      }
      continue;
    }
    if (!(names_set && query_names_set(s, q)) && !(names_field && query_names_field(s, q))) continue;  // (it went with an EMPTY form's clauses)
    if (st.set_q.empty()) st.set_q.assign(n_queries, 0);
    st.set_q[qi] = 1;
    ++st.n_set;
    if (q.mode == TQ_MODE_BOOL) continue;
    if (st.eff.empty()) st.eff.assign(queries, queries + n_queries);
    st.set_occurs.emplace_back();
    st.set_occurs.back().fill(q.mode == TQ_MODE_AND ? (uint8_t)TQ_MUST : (uint8_t)TQ_SHOULD);
    tq_query &v = st.eff[qi];
    v.mode = TQ_MODE_BOOL;
    v.occurs = st.set_occurs.back().data();
    v.clause_of = v.nested_occurs = v.clause_min_should = v.atom_of = nullptr;
    v.min_should_match = 0;
  }
  return TQ_OK;
}

// The pinned rows of a host-output batch: scores | docs | counts, each 256-byte aligned; returns the total bytes.
size_t host_rows_layout(uint32_t n_queries, uint32_t out_stride, size_t &o_docs, size_t &o_counts) {
  const size_t n = (size_t)n_queries * out_stride;
  o_docs = (n * sizeof(float) + 255) & ~(size_t)255;
  o_counts = (o_docs + n * sizeof(uint32_t) + 255) & ~(size_t)255;
  return o_counts + (size_t)n_queries * sizeof(uint32_t);
}

}  // namespace

int search_batch_impl(tq_segment *s, const tq_query *queries, uint32_t n_queries,
                      uint32_t out_stride, float *d_out_scores, uint32_t *d_out_docs,
                      uint32_t *d_out_counts, void *hip_stream, const CallOpts &co, uint32_t *d_out_segment_ords,
                      uint32_t segment_ord) {
  if (!s || (!queries && n_queries) || !d_out_scores || !d_out_docs || !d_out_counts)
    return fail(TQ_ERR_INVALID, "tq_search_batch: null argument");
  if (n_queries == 0) return TQ_OK;
  AllStrip strip;
  int rc = strip_all_clauses(s, queries, n_queries, strip);
  if (rc != TQ_OK) return rc;
  if (!strip.eff.empty()) queries = strip.eff.data();
  Batch b{s, queries, n_queries, out_stride, d_out_scores, d_out_docs, d_out_counts, hip_stream, co, d_out_segment_ords, segment_ord};
  b.n_all_queries = strip.n_all_based;
  b.set_q = strip.n_set ? strip.set_q.data() : nullptr;
  b.slop_q = strip.slop_q.empty() ? nullptr : strip.slop_q.data();
  rc = plan_batch(b);
  // a shared launch's result lists over the budget even with the longest tasks: the same batch again, that family
  // through the per-query kernels
  while (rc != TQ_OK && b.replan) {
    drop_leader_mats(b);
    b = Batch{s, queries, n_queries, out_stride, d_out_scores, d_out_docs, d_out_counts, hip_stream, b.co, d_out_segment_ords, segment_ord};
    b.n_all_queries = strip.n_all_based;
    b.set_q = strip.n_set ? strip.set_q.data() : nullptr;
    b.slop_q = strip.slop_q.empty() ? nullptr : strip.slop_q.data();
    rc = plan_batch(b);
  }
  struct DropMats {  // (whatever ends the call before fill_leader_mats has run)
    Batch &b;
    ~DropMats() { drop_leader_mats(b); }
  } drop_mats{b};
  if (rc != TQ_OK) return rc;
  // From here to the event behind the batch's last kernel the device's shared scratch is this batch's.
  b.sc = s->dscratch;
  std::unique_lock<std::mutex> scratch_lock(b.sc->m);
  if ((rc = lay_out_stage(b)) != TQ_OK || (rc = fill_stage(b)) != TQ_OK || (rc = order_batch(b)) != TQ_OK || (rc = fill_leader_mats(b)) != TQ_OK) return rc;
  DrainOnError drain_on_error{s, b.st};
  if ((rc = enqueue_copy(b)) != TQ_OK || (rc = zero_batch_buffers(b)) != TQ_OK || (rc = launch_groups(b)) != TQ_OK ||
      (rc = launch_merges(b)) != TQ_OK || (rc = finish_batch(b)) != TQ_OK)
    return rc;
  drain_on_error.armed = false;
  s->host_ms_sum += std::chrono::duration<double, std::milli>((Clock::now() - b.t0) - (b.t_waited - b.t_laid)).count();
  ++s->host_ms_n;
  return TQ_OK;
}

int resolve_opts(const tq_segment *s, const tq_search_opts *o, CallOpts &co) {
  // (atomic loads: tq_submit resolves a call's options without the segment lock)
  co.exhaustive = __atomic_load_n(&s->opt.exhaustive, __ATOMIC_RELAXED) != 0;
  uint32_t ppm = (uint32_t)__atomic_load_n(&s->opt.bound_slack_ppm, __ATOMIC_RELAXED);
  if (o) {
    if (o->exhaustive == 0 || o->exhaustive == 1)
      co.exhaustive = o->exhaustive != 0;
    else if (o->exhaustive != -1)
      return fail(TQ_ERR_INVALID, "tq_search_opts.exhaustive must be -1, 0 or 1");
    if (o->bound_slack_ppm != TQ_OPT_DEFAULT) ppm = o->bound_slack_ppm;
    if (ppm > 1000000000u) return fail(TQ_ERR_INVALID, "bound_slack_ppm above 1e9");
  }
  co.bound_slack = 1.0f + (float)ppm * 1e-6f;
  return TQ_OK;
}

int search_batch_host(tq_segment *s, const tq_query *queries, uint32_t n_queries,
                      uint32_t out_stride, float *out_scores, uint32_t *out_docs,
                      uint32_t *out_counts, const CallOpts &co) {
  if (!s || !out_scores || !out_docs || !out_counts)
    return fail(TQ_ERR_INVALID, "tq_search_batch: null argument");
  if (n_queries == 0) return TQ_OK;
  HIP_TRY(hipSetDevice(s->device));
  // The merge kernels write the rows STRAIGHT into pinned host memory (hipHostMalloc memory is mapped into the
  // device's address space): scores | docs | counts in one buffer, no device-to-host copy operations — three copies into
  // the caller's pageable arrays were three staged, blocking operations (and an asynchronous copy into pinned memory
  // now and then held the calling thread for 7 ms, tantivy_amd/distributed.py).
  const size_t n = (size_t)n_queries * out_stride;
  size_t o_docs, o_counts;
  const size_t o_over = (host_rows_layout(n_queries, out_stride, o_docs, o_counts) + 255) & ~(size_t)255;  // (the overflow words of sloppy phrases)
  int rc = s->h_out.ensure(o_over + (size_t)n_queries * sizeof(uint32_t));
  if (rc != TQ_OK) return rc;
  uint8_t *h = (uint8_t *)s->h_out.p;
  CallOpts co_over = co;
  co_over.h_slop_over = (uint32_t *)(h + o_over);
  rc = search_batch_impl(s, queries, n_queries, out_stride, (float *)h, (uint32_t *)(h + o_docs),
                         (uint32_t *)(h + o_counts), nullptr, co_over);
  if (rc != TQ_OK) return rc;
  HIP_TRY(hipStreamSynchronize(s->stream));
  memcpy(out_scores, h, n * sizeof(float));
  memcpy(out_docs, h + o_docs, n * sizeof(uint32_t));
  memcpy(out_counts, h + o_counts, (size_t)n_queries * sizeof(uint32_t));
  if (co.defer_slop_verdict) {
    if (s->last_batch_slop) s->slop_over_host.assign((const uint32_t *)(h + o_over), (const uint32_t *)(h + o_over) + n_queries);
    return TQ_OK;
  }
  // (the rows above are written and valid for every other query: the caller falls back for the one named)
  return s->last_batch_slop ? slop_overflow_verdict("tq_search_batch", (const uint32_t *)(h + o_over), n_queries) : TQ_OK;
}
int search_batch_host_begin(tq_segment *s, const tq_query *queries, uint32_t n_queries, uint32_t out_stride,
                            const CallOpts &co, HostBatchSlot &slot) {
  if (!s || !n_queries) return fail(TQ_ERR_INVALID, "tq_submit: empty batch");
  HIP_TRY(hipSetDevice(s->device));
  slot.n = n_queries;
  slot.stride = out_stride;
  slot.o_slop_over = (host_rows_layout(n_queries, out_stride, slot.o_docs, slot.o_counts) + 255) & ~(size_t)255;
  int rc = slot.out.ensure(slot.o_slop_over + (size_t)n_queries * sizeof(uint32_t));
  if (rc != TQ_OK) return rc;
  if (!slot.done) HIP_TRY(hipEventCreateWithFlags(&slot.done, hipEventDisableTiming));
  if (!slot.done_blocking) HIP_TRY(hipEventCreateWithFlags(&slot.done_blocking, hipEventDisableTiming | hipEventBlockingSync));
  uint8_t *h = (uint8_t *)slot.out.p;
  CallOpts co_over = co;
  co_over.h_slop_over = (uint32_t *)(h + slot.o_slop_over);
  rc = search_batch_impl(s, queries, n_queries, out_stride, (float *)h, (uint32_t *)(h + slot.o_docs),
                         (uint32_t *)(h + slot.o_counts), nullptr, co_over);
  if (rc != TQ_OK) return rc;
  slot.any_slop = s->last_batch_slop;
  // A batch of many callers is waited for asleep (an interrupt, some tens of microseconds later than a spinning wait
  // would notice): with hundreds of request threads the host's cores are what runs out first — the GPU box grants 16,
  // and a process above its quota is stopped for the rest of the 100 ms period, all its threads (p99 of 1 024 threads:
  // 92 ms) — and a core spinning for 0.7 ms per batch is one the callers do not have.  A small batch is a few callers
  // waiting for exactly this: the spinning wait.
  static const uint32_t kBlockMin = tune_u32("TQ_SUBMIT_BLOCK_MIN", 128);
  slot.blocking = n_queries >= kBlockMin;
  HIP_TRY(hipEventRecord(slot.blocking ? slot.done_blocking : slot.done, s->stream));
  return TQ_OK;
}
int search_batch_host_end(tq_segment *s, HostBatchSlot &slot) {
  (void)s;
  HIP_TRY(hipEventSynchronize(slot.blocking ? slot.done_blocking : slot.done));
  return TQ_OK;
}
}  // namespace tqi

extern "C" {

int tq_search_batch_device(tq_segment *s, const tq_query *queries, uint32_t n_queries,
                           uint32_t out_stride, float *d_out_scores, uint32_t *d_out_docs,
                           uint32_t *d_out_counts, void *hip_stream) {
  return tq_search_batch_device_opts(s, queries, n_queries, out_stride, d_out_scores, d_out_docs,
                                     d_out_counts, nullptr, hip_stream);
}

int tq_search_batch_device_opts(tq_segment *s, const tq_query *queries, uint32_t n_queries,
                                uint32_t out_stride, float *d_out_scores, uint32_t *d_out_docs,
                                uint32_t *d_out_counts, const tq_search_opts *opts,
                                void *hip_stream) {
  if (!s) return fail(TQ_ERR_INVALID, "tq_search_batch: null segment");
  try {  // (the planner allocates: nothing may unwind across the C boundary)
    TQ_SEGMENT_LOCK(s);
    CallOpts co;
    const int rc = resolve_opts(s, opts, co);
    if (rc != TQ_OK) return rc;
    return search_batch_impl(s, queries, n_queries, out_stride, d_out_scores, d_out_docs,
                             d_out_counts, hip_stream, co);
  } catch (const std::exception &e) {
    return fail(TQ_ERR_HIP, "tq_search_batch_device: %s", e.what());
  } catch (...) {
    return fail(TQ_ERR_HIP, "tq_search_batch_device: unknown exception");
  }
}

int tq_search_batch_device_rows(tq_segment *s, const tq_query *queries, uint32_t n_queries,
                                uint32_t out_stride, float *d_out_scores, uint32_t *d_out_segment_ords,
                                uint32_t *d_out_docs, uint32_t *d_out_counts, uint32_t segment_ord,
                                const tq_search_opts *opts, void *hip_stream) {
  if (!s) return fail(TQ_ERR_INVALID, "tq_search_batch: null segment");
  if (!d_out_segment_ords) return fail(TQ_ERR_INVALID, "tq_search_batch_device_rows: null argument");
  try {
    TQ_SEGMENT_LOCK(s);
    CallOpts co;
    const int rc = resolve_opts(s, opts, co);
    if (rc != TQ_OK) return rc;
    return search_batch_impl(s, queries, n_queries, out_stride, d_out_scores, d_out_docs,
                             d_out_counts, hip_stream, co, d_out_segment_ords, segment_ord);
  } catch (const std::exception &e) {
    return fail(TQ_ERR_HIP, "tq_search_batch_device_rows: %s", e.what());
  } catch (...) {
    return fail(TQ_ERR_HIP, "tq_search_batch_device_rows: unknown exception");
  }
}

int tq_search_batch(tq_segment *s, const tq_query *queries, uint32_t n_queries,
                    uint32_t out_stride, float *out_scores, uint32_t *out_docs,
                    uint32_t *out_counts) {
  return tq_search_batch_opts(s, queries, n_queries, out_stride, out_scores, out_docs, out_counts,
                              nullptr);
}

int tq_search_batch_opts(tq_segment *s, const tq_query *queries, uint32_t n_queries,
                         uint32_t out_stride, float *out_scores, uint32_t *out_docs,
                         uint32_t *out_counts, const tq_search_opts *opts) {
  if (!s) return fail(TQ_ERR_INVALID, "tq_search_batch: null segment");
  try {
    TQ_SEGMENT_LOCK(s);
    CallOpts co;
    const int rc = resolve_opts(s, opts, co);
    if (rc != TQ_OK) return rc;
    return search_batch_host(s, queries, n_queries, out_stride, out_scores, out_docs, out_counts, co);
  } catch (const std::exception &e) {
    return fail(TQ_ERR_HIP, "tq_search_batch: %s", e.what());
  } catch (...) {
    return fail(TQ_ERR_HIP, "tq_search_batch: unknown exception");
  }
}

}  // extern "C"
