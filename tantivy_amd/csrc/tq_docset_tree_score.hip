// tq_docset_tree_score.hip — the scores of the doc sets of phrase queries and nested boolean queries (the trees of
// tq_tree.hip): the pass behind tq_docset.hip's write pass that lets tq_docset_scored_batch* (option
// "docset_score_trees") take these shapes — Weight::for_each of PhraseWeight and of the `SpecializedScorer::Other` trees
// of BooleanWeight::complex_scorer (src/query/weight.rs:9-18,89-97).
//
// Row-driven, like docset_score_kernel: the rows are there already — tq_docset_tree.hip wrote the query's exact match
// bits, the count / scan / write passes turned them into ascending alive docs at tile_offs — so a workgroup owns one
// (tree query, tile of 65 536 docs), query fastest, and consecutive lanes take consecutive output positions of the tile:
// out_docs is read and out_scores written coalesced.  One lane computes one doc's score over the TqdTreeQuery record
// plan_tree_query emits, in tree_kernel's association: no atomics, nothing that depends on the order of lanes, no
// writes across workgroups.
//
// What the row proves: the doc matches and is alive.  So the top-level MustNot clauses (the planner puts them last) are
// not visited, and no verdict over the whole query and no top-k is computed.  What it does not prove is whether an
// OPTIONAL part matches: a Should clause adds its score only where it matches (its nested Must / MustNot members, its
// nested minimum, a phrase atom decided by its positions), so that part of the verdict stays.
// A phrase atom scores bm25(atom weight, norm, number of aligned positions) from the full cursor walk
// (PhraseScorer::compute_phrase_count, phrase_scorer.rs:347-587); docset_tree_score_kernel<false> (no tree of the launch
// has one) does not carry the cursors.
//
// Latency hiding: the flat pass (tq_docset_score.hip) gains 15 % from requesting the bitmap words of four lists before
// the first is used.  The same is built in here — the lists are taken TS_CHUNK at a time: every bitmap word of the chunk
// is requested first, then every tf byte, and only then are the terms added up, in list order — and measured
// (tools/bench_docset.py --trees --scores, `nested`, the pass alone): 1 / 2 / 4 / 8 lists 7.3 / 10.2 / 10.7 / 12.1 ms.
// It LOSES here (the per-term body with its atom and clause bookkeeping is unrolled TS_CHUNK times), so the default is
// one list at a time: tree_kernel's own sequence.
//
// DUPLICATED from tq_tree.hip, which stays as it is (sharing the code would change the registers of the hottest
// nested-query kernel) — keep in step with:
//   tq_tree.hip:146-186  fieldnorm, a term of a clause: bitmap word -> rank -> tf byte, 255 -> the packed tf of the block
//   tq_tree.hip:187-255  atoms: unions one level down, the cursor set-up and the count of a phrase atom
//   tq_tree.hip:256-290  must_ok / not_ok / ns >= inner_need per clause; Intersection::score (first + second + others),
//                        RequiredOptionalScorer (req + opt), SumCombiner — the order of every float addition
// The loops over clauses and terms are one loop over the terms here (chunks do not stop at clause ends); a clause is
// closed behind its last term.  tests/test_gpu_docset_tree_scored.py checks the scores against the oracle over
// tests/tree_shapes.py and bit for bit against tree_kernel's own (tq_search_batch, exhaustive).
//
// HBM model per output doc: 4 (doc) + 4 (score) + 1 (fieldnorm) bytes; per scoring list at most one 8-byte bitmap word
// per 32 docs of the segment; positions are not counted.
#include "tq_common.hpp"
#include "tq_launch.h"

namespace {

constexpr uint32_t TS_THREADS = 256;
#ifndef TQ_TREE_SCORE_CHUNK
#define TQ_TREE_SCORE_CHUNK 1
#endif
#ifndef TQ_TREE_SCORE_CHUNK_PH
#define TQ_TREE_SCORE_CHUNK_PH 1
#endif
// lists whose gathers are in flight together (experiments: see above), without / beside the position cursors — with 4
// beside the cursors the kernel takes 75 VGPRs, above tree_kernel<1, true>'s 67
template <bool PH>
constexpr uint32_t ts_chunk() { return PH ? TQ_TREE_SCORE_CHUNK_PH : TQ_TREE_SCORE_CHUNK; }

template <bool PH>
__global__ __launch_bounds__(TS_THREADS) void docset_tree_score_kernel(TqkDocsetTreeScoreParams p) {
  constexpr uint32_t TS_CHUNK = ts_chunk<PH>();
  const int lane = (int)__lane_id();
  const uint32_t q = blockIdx.x % p.n_queries, tile = blockIdx.x / p.n_queries;
  const size_t entry = (size_t)sload(p.query_of + q) * p.n_tiles + tile;
  const uint32_t tile_docs = p.tile_counts[entry];
  if (tile_docs == 0u) return;  // (uniform for the workgroup; a query the planner found empty has no docs anywhere)
  const uint64_t start = p.tile_offs[entry];
  if (start >= p.out_cap) return;  // nothing of this tile was written
  const uint32_t n = (uint32_t)(p.out_cap - start < (uint64_t)tile_docs ? p.out_cap - start : (uint64_t)tile_docs);
  const TqdTreeQuery *Q = p.queries + q;
  const uint32_t nc = sload(&Q->n_clauses);
  const float *cache = p.caches + (size_t)sload(&Q->cache_idx) * 256u;
  const uint8_t *tbase = p.table_base;
  const TqdSegment &seg = p.seg;
  // the clauses that score: Must, then Should; the MustNot clauses behind them only shaped the doc set
  uint32_t n_sc = 0;
  while (n_sc < nc && sload(Q->outer + n_sc) != TQD_ROLE_MUST_NOT) ++n_sc;
  const uint32_t t_end = sload(Q->first_term + n_sc);
  for (uint32_t base = (threadIdx.x & ~63u); base < n; base += TS_THREADS) {  // (uniform for the wavefront)
    const uint32_t j = base + (uint32_t)lane;
    uint32_t doc = 0;
    bool has = j < n;
    if (has) doc = p.out_docs[start + j];
    has = has && doc < seg.max_doc;
    const uint32_t w = doc >> 5, bit = doc & 31u;
    const float norm = cache[has ? fieldnorm_id(seg, doc) : 0u];
    float musts_first = 0.0f, musts_second = 0.0f, musts_others = 0.0f, opt = 0.0f;
    uint32_t n_must_clauses = 0;
    // the clause the terms belong to (every clause of a record holds at least one term), and its state
    uint32_t c = 0, c_end = sload(Q->first_term + 1u);
    bool must_ok = true, not_ok = true;
    uint32_t ns = 0;
    float csum = 0.0f;
    bool atom_ok = true;     // the doc holds every term of the current atom so far
    bool atom_some = false;  // ... or any of them (a union one level down)
    float atom_sum = 0.0f;   // ... and what they score together (Intersection::score / SumCombiner)
    uint32_t atom_t0 = 0;
    for (uint32_t t0 = 0; t0 < t_end; t0 += TS_CHUNK) {
      uint2 wd[TS_CHUNK];
      uint32_t tfb[TS_CHUNK];
#pragma unroll
      for (uint32_t u = 0; u < TS_CHUNK; ++u) {
        const uint32_t t = t0 + u;
        wd[u] = make_uint2(0u, 0u);
        if (t < t_end) {  // (uniform)
          const uint2 *bm = reinterpret_cast<const uint2 *>(tbase + ((uint64_t)sload(Q->dense_off + t) << 3));
          if (has) wd[u] = bm[w];
        }
      }
#pragma unroll
      for (uint32_t u = 0; u < TS_CHUNK; ++u) {
        const uint32_t t = t0 + u;
        tfb[u] = 0u;
        if (t < t_end) {
          // (a const-score leaf, atom_end bit 3, has no tf bytes: its tf8_off names the bitmap again)
          const bool scores = sload(Q->inner + t) != TQD_ROLE_MUST_NOT && !(sload(Q->atom_end + t) & 8u) && !(PH && (sload(Q->atom_end + t) & 2u));
          if (scores && ((wd[u].x >> bit) & 1u))
            tfb[u] = (tbase + ((uint64_t)sload(Q->tf8_off + t) << 3))[wd[u].y + (uint32_t)__popc(wd[u].x & ((1u << bit) - 1u))];
        }
      }
#pragma unroll
      for (uint32_t u = 0; u < TS_CHUNK; ++u) {
        const uint32_t t = t0 + u;
        if (t >= t_end) break;
        const uint32_t inner = sload(Q->inner + t);
        const uint32_t ae = sload(Q->atom_end + t);
        const bool present = has && ((wd[u].x >> bit) & 1u);
        atom_ok = atom_ok && present;
        atom_some = atom_some || present;
        if (present && (ae & 8u)) {  // a const-score leaf (a term set): its weight as given
          if (inner != TQD_ROLE_MUST_NOT) atom_sum = atom_sum + __uint_as_float(sload(Q->weight_bits + t));
        } else if (present && inner != TQD_ROLE_MUST_NOT && !(PH && (ae & 2u))) {
          const uint32_t pi = wd[u].y + (uint32_t)__popc(wd[u].x & ((1u << bit) - 1u));
          uint32_t tf = tfb[u];
          if (tf == 255u) {  // saturated byte: block record -> packed tf (tq_common.hpp)
            const TqdTermHead *h = p.terms + sload(Q->handle + t);
            TermRef tr{};
            tr.rec = h->rec;
            tr.tail_tfs = h->tail_tfs;
            tr.payload_base = h->payload_base;
            tr.has_freq = h->has_freq & 1u;
            const uint4 r = tr.rec[pi >> 7];
            tf = block_tf_at(seg.idx, tr, make_uint2(r.y, r.z), pi & 127u);
          }
          atom_sum = atom_sum + bm25(__uint_as_float(sload(Q->weight_bits + t)), norm, tf);
        }
        if (ae & 1u) {
          if (ae & 4u) atom_ok = atom_some;  // (a union: the present terms' scores are already in atom_sum)
          if constexpr (PH) {
            if (ae & 2u) {  // a PhraseQuery: count the positions where its terms line up (lanes that hold them all)
              uint32_t cnt = 0;
              if (atom_ok) {
                PosCursor cur[TQK_TREE_PHRASE_TERMS];
                const uint32_t n_ph = t + 1u - atom_t0;
#pragma unroll
                for (uint32_t m = 0; m < TQK_TREE_PHRASE_TERMS; ++m) {
                  cur[m].valid = false;
                  cur[m].idx = cur[m].end = cur[m].cur = 0;
                  if (m < n_ph) {
                    const uint32_t tt = atom_t0 + m;
                    const uint2 wm = reinterpret_cast<const uint2 *>(tbase + ((uint64_t)sload(Q->dense_off + tt) << 3))[w];
                    const uint32_t pi = wm.y + (uint32_t)__popc(wm.x & ((1u << bit) - 1u));
                    // the four tf bytes of the posting's group of four + the group's directory entry
                    const uint32_t tw = *reinterpret_cast<const uint32_t *>(tbase + ((uint64_t)sload(Q->tf8_off + tt) << 3) + (pi & ~3u));
                    const uint32_t dv = reinterpret_cast<const uint32_t *>(tbase + ((uint64_t)sload(Q->dir_off + tt) << 3))[pi >> 2];
                    const uint32_t l0 = pi & 3u;
                    const uint32_t b0 = tw & 0xFFu, b1 = (tw >> 8) & 0xFFu, b2 = (tw >> 16) & 0xFFu, b3 = tw >> 24;
                    uint32_t tf = l0 == 0u ? b0 : (l0 == 1u ? b1 : (l0 == 2u ? b2 : b3));
                    uint32_t ex = (l0 > 0u ? b0 : 0u) + (l0 > 1u ? b1 : 0u) + (l0 > 2u ? b2 : 0u);
                    if (tf == 255u || (l0 > 0u && b0 == 255u) || (l0 > 1u && b1 == 255u) || (l0 > 2u && b2 == 255u)) {
                      const TqdTermHead *h = p.terms + sload(Q->handle + tt);  // a saturated byte: the packed values
                      TermRef tr{};
                      tr.rec = h->rec;
                      tr.tail_tfs = h->tail_tfs;
                      tr.payload_base = h->payload_base;
                      tr.has_freq = h->has_freq & 1u;
                      tr.n_tail = h->n_tail;
                      group_tfs(seg.idx, tr, tr.rec[pi >> 7], pi & 127u, tf, ex);
                    }
                    const TqdTerm *term = p.terms + sload(Q->handle + tt);
                    const uint32_t fp = dv + ex;  // index of the doc's first position in the term's stream
                    cur[m].idx = fp + 1u;
                    cur[m].end = fp + tf;
                    cur[m].valid = tf >= 1u;
                    if (cur[m].valid) cur[m].cur = sload(Q->phrase_off + tt) + position_delta(seg.pos, term, fp);
                  }
                }
                bool done = false;
                while (cur[0].valid && !done) {
                  const uint32_t av = cur[0].cur;
                  bool okv = true;
#pragma unroll
                  for (uint32_t m = 1; m < TQK_TREE_PHRASE_TERMS; ++m) {
                    if (m < n_ph && !done) {
                      const TqdTerm *term = p.terms + sload(Q->handle + atom_t0 + m);
                      while (cur[m].valid && cur[m].cur < av) pos_advance(cur[m], seg.pos, term);
                      if (!cur[m].valid)
                        done = true;
                      else if (cur[m].cur != av)
                        okv = false;
                    }
                  }
                  if (done) break;
                  if (okv) {
                    ++cnt;
#pragma unroll
                    for (uint32_t m = 1; m < TQK_TREE_PHRASE_TERMS; ++m)
                      if (m < n_ph) pos_advance(cur[m], seg.pos, p.terms + sload(Q->handle + atom_t0 + m));
                  }
                  pos_advance(cur[0], seg.pos, p.terms + sload(Q->handle + atom_t0));
                }
              }
              atom_ok = cnt > 0u;
              atom_sum = atom_ok ? bm25(__uint_as_float(sload(Q->weight_bits + atom_t0)), norm, cnt) : 0.0f;
            }
          }
          if (inner == TQD_ROLE_MUST_NOT) {
            not_ok = not_ok && !atom_ok;
          } else {
            if (inner == TQD_ROLE_MUST) must_ok = must_ok && atom_ok;
            if (atom_ok) {
              if (inner == TQD_ROLE_SHOULD) ++ns;
              csum = csum + atom_sum;
            }
          }
          atom_ok = true;
          atom_some = false;
          atom_sum = 0.0f;
          atom_t0 = t + 1u;
        }
        if (t + 1u == c_end) {  // (uniform) the clause is complete
          if (sload(Q->outer + c) == TQD_ROLE_MUST) {  // Intersection::score: left + right + sum(others), clauses cheapest first
            if (n_must_clauses == 0u)
              musts_first = csum;
            else if (n_must_clauses == 1u)
              musts_second = csum;
            else
              musts_others = musts_others + csum;
            ++n_must_clauses;  // (the row proves that it matches)
          } else if (has && must_ok && not_ok && ns >= sload(Q->inner_need + c)) {
            opt = opt + csum;  // a Should clause that matches adds its score (SumCombiner / RequiredOptionalScorer)
          }
          ++c;
          c_end = c < n_sc ? sload(Q->first_term + c + 1u) : 0xFFFFFFFFu;
          must_ok = not_ok = true;
          ns = 0;
          csum = 0.0f;
        }
      }
    }
    float s = musts_first;
    if (n_must_clauses >= 2u) s = s + musts_second;
    if (n_must_clauses >= 3u) s = s + musts_others;
    s = n_must_clauses ? s + opt : opt;
    if (has && start + j < p.out_cap) p.out_scores[start + j] = s;
  }
}

}  // namespace

hipError_t tqk_launch_docset_tree_score(const TqkDocsetTreeScoreParams &p, hipStream_t st) {
  if (!p.n_tiles || !p.n_queries) return hipSuccess;
  const dim3 grid(p.n_tiles * p.n_queries), block(TS_THREADS);
  if (p.any_phrase)
    docset_tree_score_kernel<true><<<grid, block, 0, st>>>(p);
  else
    docset_tree_score_kernel<false><<<grid, block, 0, st>>>(p);
  return hipGetLastError();
}
