// tq_docset_tree.hip — the exact match bits of phrase queries and nested boolean queries (the trees of tq_tree.hip), one
// result bitmap of the doc-set batch's scratch per query: what lets tq_docset_batch* (option "docset_trees") take these
// shapes.  To the count / scan / write passes of tq_docset.hip such a query is then one Must list "that is bits in batch
// scratch", like a list without a bitmap of its own scattered by count_scatter_kernel.
//
// Geometry of tree_kernel: a 64-lane workgroup per (query, tile of TQK_TREE_TILE_WORDS words), query fastest, one lane
// per 32-doc word; the queries are the TqdTreeQuery records plan_tree_query emits (part_start = the result slot).
// Per word the bitmap expression of the tree AND the alive word.  Without a phrase atom (PH = false) that word is the
// result.  With one (PH = true) it only proposes docs: a phrase atom entered it as the AND of its lists under positive
// polarity and as nothing under an odd number of MustNots, and every proposed doc gets the exact per-doc verdict — a
// phrase atom decided by walking one position cursor per term until the first position where they line up
// (PhraseScorer::phrase_match, phrase_scorer.rs:347-385).  Nothing is scored: no fieldnorm, no tf of a non-phrase
// term, no BM25, no top-k.  Every lane stores its word with a plain store: one writer per word, no atomics, and the
// result does not depend on the other queries of the batch.
//
// DUPLICATED from tq_tree.hip, which stays as it is (sharing the code would change the registers of the hottest
// nested-query kernel for no gain here) — keep in step with:
//   tq_tree.hip:36-73    SlicedCount
//   tq_tree.hip:96-138   the bitmap expression (clauses, atoms, unions one level down, phrase polarity, the alive word)
//   tq_tree.hip:141-292  the per-doc verdict (must_ok / not_ok / ns >= inner_need per clause, then all_must && !any_not
//                        && n_should_clauses >= top_need) and the cursor set-up of a phrase atom, without the scoring
// tests/test_gpu_docset_tree.py checks both against the oracle over tests/tree_shapes.py, as tests/test_gpu_tree.py
// does for tree_kernel.
//
// HBM model: 8 B per list per 32 docs read, 4 B per 32 docs written; the positions of the proposed docs on top.
#include "tq_common.hpp"
#include "tq_launch.h"

namespace {

constexpr uint32_t TREE_TILE_WORDS = TQK_TREE_TILE_WORDS;

// bit-sliced counter of one-bit-per-doc inputs (4 planes), SATURATING at 15 (tq_tree.hip:36-73)
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

template <bool PH>
__global__ __launch_bounds__(64) void docset_tree_bits_kernel(TqkDocsetTreeParams p) {
  const int lane = (int)__lane_id();
  const uint32_t q = blockIdx.x % p.n_queries, tile = blockIdx.x / p.n_queries;
  const TqdTreeQuery *Q = p.queries + q;
  const uint32_t nt = sload(&Q->n_terms), nc = sload(&Q->n_clauses);
  const uint32_t top_need = sload(&Q->top_need), top_has_must = sload(&Q->top_has_must);
  const uint8_t *tbase = p.table_base;
  const TqdSegment seg = p.seg;
  uint32_t *out = p.bits + (size_t)sload(&Q->part_start) * p.words_per_list;
  const uint32_t w_end = (tile + 1u) * TREE_TILE_WORDS < p.n_words ? (tile + 1u) * TREE_TILE_WORDS : p.n_words;
  if (nt == 0 || nc == 0) {  // (a query the planner found empty: an absent Must term, too few Should clauses, ...)
    for (uint32_t w = tile * TREE_TILE_WORDS + (uint32_t)lane; w < w_end; w += 64u) out[w] = 0u;
    return;
  }
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
      if (outer_c == TQD_ROLE_MUST)
        top_must &= cm;
      else if (outer_c == TQD_ROLE_MUST_NOT)
        top_not |= cm;
      else
        top_should.add(cm);
    }
    uint32_t match = (top_has_must ? top_must : 0xFFFFFFFFu) & ~top_not & top_should.at_least(top_need);
    if (!in) match = 0u;
    if (seg.alive) match &= in ? reinterpret_cast<const uint32_t *>(seg.alive)[w] : 0u;  // AliveBitSet (alive_bitset.rs:58-61)
    if constexpr (PH) {
      // ---- the word only proposed its docs: every lane takes the lowest doc of its word until none has one left
      // (the loops over clauses and terms stay wave-uniform: the descriptor is read through scalar loads)
      uint32_t rest = match;
      while (__ballot(rest != 0u)) {
        const bool has = rest != 0u;
        const uint32_t bit = has ? (uint32_t)__builtin_ctz(rest) : 0u;
        rest &= rest - 1u;
        bool all_must = true, any_not = false;
        uint32_t n_should_clauses = 0;
        for (uint32_t c = 0; c < nc; ++c) {
          const uint32_t t0 = sload(Q->first_term + c), t1 = sload(Q->first_term + c + 1u);
          const uint32_t outer = sload(Q->outer + c);
          bool must_ok = true, not_ok = true;
          uint32_t ns = 0;
          bool atom_ok = true;     // the doc holds every term of the current atom so far
          bool atom_some = false;  // ... or any of them (a union one level down)
          uint32_t atom_t0 = t0;
          for (uint32_t t = t0; t < t1; ++t) {
            const uint32_t inner = sload(Q->inner + t);
            const uint32_t ae = sload(Q->atom_end + t);
            const uint2 *bm = reinterpret_cast<const uint2 *>(tbase + ((uint64_t)sload(Q->dense_off + t) << 3));
            uint32_t wx = 0u;
            if (has) wx = bm[w].x;
            const bool present = (wx >> bit) & 1u;
            atom_ok = atom_ok && present;
            atom_some = atom_some || present;
            if (!(ae & 1u)) continue;
            if (ae & 4u) atom_ok = atom_some;
            if (ae & 2u) {  // a PhraseQuery: is there a position where its terms line up (lanes that hold them all)
              bool found = false;
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
                while (cur[0].valid && !done && !found) {
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
                  found = okv;  // the first aligned position decides (phrase_match: no count is needed)
                  pos_advance(cur[0], seg.pos, p.terms + sload(Q->handle + atom_t0));
                }
              }
              atom_ok = found;
            }
            if (inner == TQD_ROLE_MUST_NOT) {
              not_ok = not_ok && !atom_ok;
            } else {
              if (inner == TQD_ROLE_MUST) must_ok = must_ok && atom_ok;
              if (atom_ok && inner == TQD_ROLE_SHOULD) ++ns;
            }
            atom_ok = true;
            atom_some = false;
            atom_t0 = t + 1u;
          }
          const bool cmatch = has && must_ok && not_ok && ns >= sload(Q->inner_need + c);
          if (outer == TQD_ROLE_MUST)
            all_must = all_must && cmatch;
          else if (outer == TQD_ROLE_MUST_NOT)
            any_not = any_not || cmatch;
          else if (cmatch)
            ++n_should_clauses;
        }
        const bool doc_ok = has && all_must && !any_not && n_should_clauses >= top_need;
        if (has && !doc_ok) match &= ~(1u << bit);
      }
    }
    if (in) out[w] = match;
  }
}

}  // namespace

hipError_t tqk_launch_docset_tree(const TqkDocsetTreeParams &p, hipStream_t st) {
  const uint32_t tiles = tqk_tree_tiles(p.n_words);
  if (!tiles || !p.n_queries) return hipSuccess;
  const dim3 grid(tiles * p.n_queries), block(64);
  if (p.any_phrase)
    docset_tree_bits_kernel<true><<<grid, block, 0, st>>>(p);
  else
    docset_tree_bits_kernel<false><<<grid, block, 0, st>>>(p);
  return hipGetLastError();
}
