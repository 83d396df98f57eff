// tq_tree_fields.hip — tree_kernel (tq_tree.hip) over the lists of SEVERAL fields of a multi-field segment
// (tq_fields.cpp, include/tantivy_amd.h "multi-field segments"): the same bitmap expression, the same scoring stage and
// the same sums — per-LIST norms in place of the per-doc norm.  A duplicate of tq_tree.hip's kernel in the way
// tq_docset_tree.hip is one, so that the single-field instantiations stay the code they were; read tq_tree.hip for what
// the stages do.  What differs:
//   - the field of list t rides in bits 4..6 of TqdTreeQuery::atom_end[t] (scalar loads: every field lookup is
//     wave-uniform), the fieldnorm pointers of fields 1.. in the launch parameters (TqkTreeFieldsParams);
//   - list t of field f scores under caches[(cache_idx + f) * 256 + fn_f[doc]] (no fieldnorm file: the constant id);
//   - a doc's fieldnorm bytes — one per field the query names — are gathered together in front of the lists' bitmap
//     gathers, not one dependent round trip per list (tq_fields.h);
//   - a phrase atom scores under the norm of its terms' field; a union atom or clause sums terms of different fields,
//     each under its own norm, in the existing order.
// A query of field-0 lists alone that rides in such a launch scores bit for bit what tree_kernel gives it.
#include "tq_common.hpp"
#include "tq_launch.h"
#include "tq_fields.h"

namespace {

constexpr uint32_t TREE_TILE_WORDS = TQK_TREE_TILE_WORDS;  // bitmap words per (query, tile) wavefront

// bit-sliced counter of one-bit-per-doc inputs (4 planes), SATURATING at 15: add, and "count >= m" for m <= 15.
// (A query holds up to TQ_MAX_TERMS = 16 Should inputs on one level: without the saturation a doc that held all 16
// wrapped to 0 and fell out of the doc set — the best-scoring doc of the query.)
struct SlicedCount {
  uint32_t p0 = 0, p1 = 0, p2 = 0, p3 = 0;
  __device__ __forceinline__ void add(uint32_t x) {
    uint32_t c = p0 & x;
    p0 ^= x;
    x = c;
    c = p1 & x;
    p1 ^= x;
    x = c;
    c = p2 & x;
    p2 ^= x;
    x = c;
    c = p3 & x;  // the carry out of the top plane: the count sticks at 15
    p3 ^= x;
    p0 |= c;
    p1 |= c;
    p2 |= c;
    p3 |= c;
  }
  __device__ __forceinline__ uint32_t at_least(uint32_t m) const {  // m wave-uniform, 0..15
    if (m == 0u) return 0xFFFFFFFFu;
    uint32_t gt = 0u, eq = 0xFFFFFFFFu;
    const uint32_t pl[4] = {p0, p1, p2, p3};
#pragma unroll
    for (int i = 3; i >= 0; --i) {
      if ((m >> i) & 1u) {
        eq &= pl[i];
      } else {
        gt |= eq & pl[i];
        eq &= ~pl[i];
      }
    }
    return gt | eq;
  }
};

template <int KPL, bool PH>
__global__ __launch_bounds__(64) void tree_fields_kernel(TqkTreeFieldsParams pp) {
  const TqkTreeParams &p = pp.base;
  const int lane = (int)__lane_id();
  const uint32_t q = blockIdx.x % p.n_queries, tile = blockIdx.x / p.n_queries;
  const TqdTreeQuery *Q = p.queries + q;
  const uint32_t nt = sload(&Q->n_terms), nc = sload(&Q->n_clauses), k = sload(&Q->k);
  const uint32_t top_need = sload(&Q->top_need), top_has_must = sload(&Q->top_has_must);
  const float *cache = p.caches + (size_t)sload(&Q->cache_idx) * 256u;
  const uint8_t *tbase = p.table_base;
  const TqdSegment seg = p.seg;
  TopK<KPL> tk;
  tk.reset(k);
  uint32_t n_matches = 0;
  uint32_t fmask = 0u;  // the fields the query's lists belong to
  for (uint32_t t = 0; t < nt; ++t) fmask |= 1u << ((sload(Q->atom_end + t) >> 4) & 7u);
  if (nt == 0 || nc == 0) {  // (a query the planner found empty: an absent Must term, too few Should clauses, ...)
    flush_partial(tk, sload(&p.sinks->partials), sload(&Q->part_start) + tile, lane);
    return;
  }
  const uint32_t w_end = (tile + 1u) * TREE_TILE_WORDS < p.n_words ? (tile + 1u) * TREE_TILE_WORDS : p.n_words;
  for (uint32_t w0 = tile * TREE_TILE_WORDS; w0 < w_end; w0 += 64u) {
    const uint32_t w = w0 + (uint32_t)lane;
    const bool in = w < w_end;
    // ---- the doc set of 32 docs per lane: clause by clause, then the clauses one level up
    uint32_t top_must = 0xFFFFFFFFu, top_not = 0u;
    SlicedCount top_should;
    for (uint32_t c = 0; c < nc; ++c) {
      const uint32_t t0 = sload(Q->first_term + c), t1 = sload(Q->first_term + c + 1u);
      const uint32_t outer_c = sload(Q->outer + c);
      uint32_t must = 0xFFFFFFFFu, nots = 0u;
      SlicedCount should;
      uint32_t atom = 0xFFFFFFFFu;  // the docs that hold every term of the current atom so far
      uint32_t atom_any = 0u;       // ... or any of them (a union one level down: atom_end bit 2)
      for (uint32_t t = t0; t < t1; ++t) {
        const uint2 *bm = reinterpret_cast<const uint2 *>(tbase + ((uint64_t)sload(Q->dense_off + t) << 3));
        const uint32_t bits = in ? bm[w].x : 0u;
        atom &= bits;
        atom_any |= bits;
        const uint32_t ae = sload(Q->atom_end + t);
        if (!(ae & 1u)) continue;
        if (ae & 4u) atom = atom_any;
        atom_any = 0u;
        const uint32_t inner = sload(Q->inner + t);
        if constexpr (PH) {  // a phrase under an odd number of MustNots must not remove docs it only MAY hold
          if ((ae & 2u) && ((outer_c == TQD_ROLE_MUST_NOT) != (inner == TQD_ROLE_MUST_NOT))) atom = 0u;
        }
        if (inner == TQD_ROLE_MUST)
          must &= atom;
        else if (inner == TQD_ROLE_MUST_NOT)
          nots |= atom;
        else
          should.add(atom);
        atom = 0xFFFFFFFFu;
      }
      const uint32_t cm = must & ~nots & should.at_least(sload(Q->inner_need + c));
      const uint32_t outer = outer_c;
      if (outer == TQD_ROLE_MUST)
        top_must &= cm;
      else if (outer == TQD_ROLE_MUST_NOT)
        top_not |= cm;
      else
        top_should.add(cm);
    }
    uint32_t match = (top_has_must ? top_must : 0xFFFFFFFFu) & ~top_not & top_should.at_least(top_need);
    if (!in) match = 0u;
    if (seg.alive) match &= in ? reinterpret_cast<const uint32_t *>(seg.alive)[w] : 0u;  // AliveBitSet (alive_bitset.rs:58-61)
    if constexpr (!PH) n_matches += (uint32_t)__popc(match);
    // ---- score the matching docs: every lane takes the lowest doc of its word until none has one left
    while (__ballot(match != 0u)) {
      const bool has = match != 0u;
      const uint32_t bit = has ? (uint32_t)__builtin_ctz(match) : 0u;
      match &= match - 1u;
      const uint32_t doc = (w << 5) | bit;
      // the doc's norm under every field of the query: independent gathers, issued together
      TQ_FIELD_NORMS(cache, fmask, seg.fieldnorm, pp.fn, seg.const_fieldnorm_id, has, doc);
      float musts_first = 0.0f, musts_second = 0.0f, musts_others = 0.0f, opt = 0.0f;
      uint32_t n_must_clauses = 0;
      bool all_must = true, any_not = false;  // (PH: the doc's own verdict)
      uint32_t n_should_clauses = 0;
      for (uint32_t c = 0; c < nc; ++c) {
        const uint32_t t0 = sload(Q->first_term + c), t1 = sload(Q->first_term + c + 1u);
        const uint32_t outer = sload(Q->outer + c);
        if (!PH && outer == TQD_ROLE_MUST_NOT) continue;  // (the doc set already excludes them)
        bool must_ok = true, not_ok = true;
        uint32_t ns = 0;
        float csum = 0.0f;
        bool atom_ok = true;    // the doc holds every term of the current atom so far
        bool atom_some = false; // ... or any of them (a union one level down)
        float atom_sum = 0.0f;  // ... and what they score together (Intersection::score / SumCombiner)
        uint32_t atom_t0 = t0;
        for (uint32_t t = t0; t < t1; ++t) {
          const uint32_t inner = sload(Q->inner + t);
          const uint32_t ae = sload(Q->atom_end + t);
          const uint2 *bm = reinterpret_cast<const uint2 *>(tbase + ((uint64_t)sload(Q->dense_off + t) << 3));
          uint2 wd = make_uint2(0u, 0u);
          if (has) wd = bm[w];
          const bool present = has && ((wd.x >> bit) & 1u);
          atom_ok = atom_ok && present;
          atom_some = atom_some || present;
          if (present && (ae & 8u)) {  // a const-score leaf (a term set): its weight as given, neither rank nor tf
            if (inner != TQD_ROLE_MUST_NOT) atom_sum = atom_sum + __uint_as_float(sload(Q->weight_bits + t));
          } else if (present && inner != TQD_ROLE_MUST_NOT && !(PH && (ae & 2u))) {
            const uint32_t pi = wd.y + (uint32_t)__popc(wd.x & ((1u << bit) - 1u));
            uint32_t tf = (tbase + ((uint64_t)sload(Q->tf8_off + t) << 3))[pi];
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
            atom_sum = atom_sum + bm25(__uint_as_float(sload(Q->weight_bits + t)), TQ_FIELD_NORM_OF((ae >> 4) & 7u), tf);
          }
          if (!(ae & 1u)) continue;
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
              atom_sum = atom_ok ? bm25(__uint_as_float(sload(Q->weight_bits + atom_t0)), TQ_FIELD_NORM_OF((ae >> 4) & 7u), cnt) : 0.0f;
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
        const bool cmatch = has && must_ok && not_ok && ns >= sload(Q->inner_need + c);
        if (outer == TQD_ROLE_MUST) {  // Intersection::score: left + right + sum(others), clauses cheapest first
          if (n_must_clauses == 0u)
            musts_first = csum;
          else if (n_must_clauses == 1u)
            musts_second = csum;
          else
            musts_others = musts_others + csum;
          ++n_must_clauses;
          all_must = all_must && cmatch;
        } else if (outer == TQD_ROLE_MUST_NOT) {
          any_not = any_not || cmatch;
        } else if (cmatch) {
          opt = opt + csum;  // a Should clause that matches adds its score (SumCombiner / RequiredOptionalScorer)
          ++n_should_clauses;
        }
      }
      float s = musts_first;
      if (n_must_clauses >= 2u) s = s + musts_second;
      if (n_must_clauses >= 3u) s = s + musts_others;
      s = n_must_clauses ? s + opt : opt;
      if constexpr (PH) {  // the bitmap expression only proposed the doc
        const bool doc_ok = has && all_must && !any_not && n_should_clauses >= top_need;
        n_matches += doc_ok ? 1u : 0u;
        tk.offer(doc_ok, make_key(s, doc), lane);
      } else {
        tk.offer(has, make_key(s, doc), lane);
      }
    }
  }
  flush_partial(tk, sload(&p.sinks->partials), sload(&Q->part_start) + tile, lane);
  for (int off = 32; off > 0; off >>= 1) n_matches += __shfl_down(n_matches, off, 64);
  if (lane == 0 && n_matches) {
    atomicAdd(sload(&p.sinks->query_matches) + sload(&p.sinks->out_index)[q], n_matches);
    atomicAdd(sload(&p.sinks->match_counter), (unsigned long long)n_matches);
  }
}

}  // namespace

template <bool PH>
static void launch_tree_fields_t(const TqkTreeFieldsParams &p, int kpl, dim3 grid, dim3 block, hipStream_t st) {
  switch (kpl) {  // (the partial lists' stride is kpl * 64 keys: the same instantiations as the single-field launch)
    case 1: tree_fields_kernel<1, PH><<<grid, block, 0, st>>>(p); break;
    case 2: tree_fields_kernel<2, PH><<<grid, block, 0, st>>>(p); break;
    case 4: tree_fields_kernel<4, PH><<<grid, block, 0, st>>>(p); break;
    default: tree_fields_kernel<16, PH><<<grid, block, 0, st>>>(p); break;
  }
}
hipError_t tqk_launch_tree_fields(const TqkTreeFieldsParams &p, int kpl, hipStream_t st) {
  const uint32_t tiles = tqk_tree_tiles(p.base.n_words);
  if (!tiles || !p.base.n_queries) return hipSuccess;
  const dim3 grid(tiles * p.base.n_queries), block(64);
  if (p.base.any_phrase)
    launch_tree_fields_t<true>(p, kpl, grid, block, st);
  else
    launch_tree_fields_t<false>(p, kpl, grid, block, st);
  return hipGetLastError();
}
