// tq_phrase_slop.hip — PhraseQuery with slop > 0 (TQ_MODE_PHRASE, tq_query.slop): the reference's
// sloppy PhraseScorer (phrase_scorer.rs: intersection_count_with_slop, intersection_exists_with_slop,
// intersection_count_with_carrying_slop under compute_phrase_match / compute_phrase_count / phrase_exists) over the
// lists' bitmaps.  It is not "the exact phrase with a window":
//   - the lists are walked in COST order (doc freq ascending, ties in phrase order: Intersection::new's stable sort) —
//     the planner (tq_phrase_slop.cpp) hands the terms over in that order, list 0 is "left";
//   - positions are adjusted by phrase_off = max_offset - term_offset, distances are |a - b| on adjusted positions;
//   - 2 lists: one streaming two-pointer walk, counting (scoring) or leaving at the first pair (not scoring);
//   - 3..8 lists: the middle lists are folded one by one into a CARRIED list of (position, slop spent), which is rebuilt
//     as a new list at every step (deduplicated against its last entry only: it may hold repeats and be non-monotone);
//     the last list is then counted against the carried list with the slop spent (scoring), or tested without it (not
//     scoring) — so the two verdicts of one doc may differ, as in the reference.
//
// Geometry of tree_kernel / docset_tree_bits_kernel: a 64-lane workgroup per (query, tile of TQK_TREE_TILE_WORDS
// words), query fastest, one lane per 32-doc word.  The word proposes AND(all lists) & alive; every proposed doc gets
// the per-doc verdict from position cursors (bitmap rank -> tf bytes + position directory -> first position index,
// then one delta at a time).  Only ONE list is streamed at a time, so a lane holds one cursor and a copy for the
// look-ahead of a carry step — a "right" list is never buffered and its tf has no limit.
//
// The carried lists: two per lane (the one being read, the one being built; swapped after each middle list) of
// TQ_SLOP_CARRY_CAP entries, in LDS, entry-major ([list][entry][lane]: the lanes of a wavefront walk their lists in
// different bank columns) — 64 x 2 x 32 x (4 + 1) bytes = 20 KB per workgroup.  LDS rather than a region of batch
// scratch: the lists are indexed per lane at run time (private arrays would go to scratch memory), are touched many
// times per candidate and never outlive it.  The 2-list instantiations (CARRY = false) declare none of it.  A
// candidate whose initial or carried list would exceed the cap bumps the query's overflow word and is left out: the
// host reports it (tq_last_batch_slop_overflows), never a silently wrong row.
//
// DUPLICATED from tq_docset_tree.hip, which stays as it is — keep in step with:
//   tq_docset_tree.hip:165-195  the cursor set-up of a phrase term (rank, the group's four tf bytes, the saturated
//                               byte through group_tfs, the position directory)
//   tq_tree.hip:302-307         the partial top-k flush and the match counters
// tests/test_gpu_phrase_slop.py checks every instantiation against tests/slop_model.py.
//
// HBM model: 8 B per list per 32 docs read (+ 4 B per 32 docs written by the bits kernel); the positions of the
// proposed docs on top.
#include "tq_common.hpp"
#include "tq_launch.h"

namespace {

constexpr uint32_t TILE_WORDS = TQK_TREE_TILE_WORDS;
constexpr uint32_t CAP = TQK_SLOP_CARRY_CAP;

struct SlopCtx {  // wave-uniform
  const TqdSlopQuery *Q;
  const TqdTerm *terms;
  const uint8_t *tbase;
  const uint8_t *idx, *pos;
};

// the positions of doc (w, bit) in list t of the query (t wave-uniform): tq_docset_tree.hip:165-195
__device__ __forceinline__ PosCursor open_cursor(const SlopCtx &c, uint32_t t, uint32_t w, uint32_t bit) {
  PosCursor cur;
  const uint2 wm = reinterpret_cast<const uint2 *>(c.tbase + ((uint64_t)sload(c.Q->dense_off + t) << 3))[w];
  const uint32_t pi = wm.y + (uint32_t)__popc(wm.x & ((1u << bit) - 1u));
  // the four tf bytes of the posting's group of four + the group's directory entry
  const uint32_t tw = *reinterpret_cast<const uint32_t *>(c.tbase + ((uint64_t)sload(c.Q->tf8_off + t) << 3) + (pi & ~3u));
  const uint32_t dv = reinterpret_cast<const uint32_t *>(c.tbase + ((uint64_t)sload(c.Q->dir_off + t) << 3))[pi >> 2];
  const uint32_t l0 = pi & 3u;
  const uint32_t b0 = tw & 0xFFu, b1 = (tw >> 8) & 0xFFu, b2 = (tw >> 16) & 0xFFu, b3 = tw >> 24;
  uint32_t tf = l0 == 0u ? b0 : (l0 == 1u ? b1 : (l0 == 2u ? b2 : b3));
  uint32_t ex = (l0 > 0u ? b0 : 0u) + (l0 > 1u ? b1 : 0u) + (l0 > 2u ? b2 : 0u);
  const TqdTerm *term = c.terms + sload(c.Q->handle + t);
  if (tf == 255u || (l0 > 0u && b0 == 255u) || (l0 > 1u && b1 == 255u) || (l0 > 2u && b2 == 255u)) {
    const TqdTermHead *h = term;  // a saturated byte: the packed values
    TermRef tr{};
    tr.rec = h->rec;
    tr.tail_tfs = h->tail_tfs;
    tr.payload_base = h->payload_base;
    tr.has_freq = h->has_freq & 1u;
    tr.n_tail = h->n_tail;
    group_tfs(c.idx, tr, tr.rec[pi >> 7], pi & 127u, tf, ex);
  }
  const uint32_t fp = dv + ex;  // index of the doc's first position in the term's stream
  cur.idx = fp + 1u;
  cur.end = fp + tf;
  cur.valid = tf >= 1u;
  cur.cur = cur.valid ? sload(c.Q->phrase_off + t) + position_delta(c.pos, term, fp) : 0u;
  return cur;
}

__device__ __forceinline__ uint32_t absdiff(uint32_t a, uint32_t b) { return a > b ? a - b : b - a; }

// ---- 2 lists: intersection_count_with_slop / intersection_exists_with_slop, both lists streamed
template <bool COUNT>
__device__ __forceinline__ uint32_t pair_walk(const SlopCtx &c, uint32_t w, uint32_t bit, uint32_t slop) {
  const TqdTerm *ta = c.terms + sload(c.Q->handle + 0), *tb = c.terms + sload(c.Q->handle + 1);
  PosCursor A = open_cursor(c, 0u, w, bit), B = open_cursor(c, 1u, w, bit);
  uint32_t n = 0;
  while (A.valid && B.valid) {
    const uint32_t a = A.cur, b = B.cur;
    if (absdiff(a, b) <= slop) {
      if (!COUNT) return 1u;
      ++n;
      // "there could be a better match": left moves to its last value <= b, then one further — the first value > b
      do pos_advance(A, c.pos, ta);
      while (A.valid && A.cur <= b);
      pos_advance(B, c.pos, tb);
    } else if (a < b) {
      pos_advance(A, c.pos, ta);
    } else {
      pos_advance(B, c.pos, tb);
    }
  }
  return n;
}

// ---- 3..8 lists: a lane's two carried lists in LDS
struct Carry {
  uint32_t *pos;  // [2][CAP][64]
  uint8_t *sp;    // [2][CAP][64]
  uint32_t lane;
  __device__ __forceinline__ uint32_t &P(uint32_t buf, uint32_t i) const { return pos[(buf * CAP + i) * 64u + lane]; }
  __device__ __forceinline__ uint8_t &S(uint32_t buf, uint32_t i) const { return sp[(buf * CAP + i) * 64u + lane]; }
};

// add_val of the reference: a value equal to the LAST one kept only lowers that entry's slop.  false = the list is full.
__device__ __forceinline__ bool carry_add(const Carry &L, uint32_t out, uint32_t &n_out, uint32_t spent, uint32_t value) {
  if (n_out && L.P(out, n_out - 1u) == value) {
    uint8_t &s = L.S(out, n_out - 1u);
    if (spent < s) s = (uint8_t)spent;
    return true;
  }
  if (n_out == CAP) return false;
  L.P(out, n_out) = value;
  L.S(out, n_out) = (uint8_t)spent;
  ++n_out;
  return true;
}

// intersection_count_with_carrying_slop(update_left = true): list t folded into the carried list `in` (n_in >= 1
// entries) -> list `1 - in`.  Returns false on overflow.
__device__ __forceinline__ bool carry_fold(const SlopCtx &c, const Carry &L, uint32_t t, uint32_t w, uint32_t bit, uint32_t slop,
                                           uint32_t in, uint32_t n_in, uint32_t &n_out) {
  const TqdTerm *term = c.terms + sload(c.Q->handle + t);
  PosCursor R = open_cursor(c, t, w, bit);
  const uint32_t out = 1u - in;
  n_out = 0;
  if (!R.valid) return true;
  uint32_t li = 0;
  for (;;) {
    const uint32_t a = L.P(in, li), sa = L.S(in, li), b = R.cur;
    const uint32_t d = sa + absdiff(a, b);
    if (d <= slop) {
      // both values stay, and every value of the smaller one's list up to the larger one
      uint32_t cur = d;
      if (a < b) {
        if (!carry_add(L, out, n_out, cur, a)) return false;
        for (uint32_t i = li; i + 1u < n_in && L.P(in, i + 1u) <= b; ++i) {
          const uint32_t nv = L.P(in, i + 1u);
          cur = sa + (b - nv);
          if (!carry_add(L, out, n_out, cur, nv)) return false;
        }
        if (!carry_add(L, out, n_out, cur, b)) return false;
      } else {
        if (!carry_add(L, out, n_out, cur, b)) return false;
        PosCursor W = R;  // the look-ahead walks a copy: the right list goes on from its NEXT value afterwards
        for (;;) {
          pos_advance(W, c.pos, term);
          if (!W.valid || W.cur > a) break;
          cur = sa + (a - W.cur);
          if (!carry_add(L, out, n_out, cur, W.cur)) return false;
        }
        if (!carry_add(L, out, n_out, cur, a)) return false;
      }
      ++li;
      pos_advance(R, c.pos, term);
    } else if (a < b) {
      ++li;
    } else {
      pos_advance(R, c.pos, term);
    }
    if (li >= n_in) {  // the rest of the right list against the LAST left value
      const uint32_t la = L.P(in, n_in - 1u), ls = L.S(in, n_in - 1u);
      while (R.valid) {
        const uint32_t nd = absdiff(la, R.cur) + ls;
        if (nd <= slop && !carry_add(L, out, n_out, nd, R.cur)) return false;
        pos_advance(R, c.pos, term);
      }
      return true;
    }
    if (!R.valid) {  // the rest of the left list against the LAST right value (an exhausted cursor keeps it)
      const uint32_t lb = R.cur;
      for (uint32_t i = li; i < n_in; ++i) {
        const uint32_t nd = absdiff(L.P(in, i), lb) + L.S(in, i);
        if (nd <= slop && !carry_add(L, out, n_out, nd, L.P(in, i))) return false;
      }
      return true;
    }
  }
}

// the last list: the count of intersection_count_with_carrying_slop(update_left = false) — the walk alone decides it —
// or intersection_exists_with_slop, which does not read the slops spent
template <bool COUNT>
__device__ __forceinline__ uint32_t carry_last(const SlopCtx &c, const Carry &L, uint32_t t, uint32_t w, uint32_t bit, uint32_t slop,
                                               uint32_t in, uint32_t n_in) {
  const TqdTerm *term = c.terms + sload(c.Q->handle + t);
  PosCursor R = open_cursor(c, t, w, bit);
  uint32_t li = 0, n = 0;
  while (li < n_in && R.valid) {
    const uint32_t a = L.P(in, li), b = R.cur;
    const uint32_t d = (COUNT ? (uint32_t)L.S(in, li) : 0u) + absdiff(a, b);
    if (d <= slop) {
      if (!COUNT) return 1u;
      ++n;
      ++li;
      pos_advance(R, c.pos, term);
    } else if (a < b) {
      ++li;
    } else {
      pos_advance(R, c.pos, term);
    }
  }
  return n;
}

// One candidate doc -> its phrase count (COUNT) or 0 / 1 (not COUNT).  *over: its initial or a carried list did not fit.
template <bool COUNT, bool CARRY>
__device__ __forceinline__ uint32_t doc_verdict(const SlopCtx &c, const Carry &L, uint32_t nt, uint32_t w, uint32_t bit, uint32_t slop, bool *over) {
  if constexpr (!CARRY) {
    return pair_walk<COUNT>(c, w, bit, slop);
  } else {
    uint32_t in = 0, n_in = 0;
    {  // the first list's own positions are the initial "left", nothing spent
      const TqdTerm *term = c.terms + sload(c.Q->handle + 0);
      PosCursor A = open_cursor(c, 0u, w, bit);
      if (A.valid && A.end - A.idx + 1u > CAP) {
        *over = true;
        return 0u;
      }
      while (A.valid) {
        L.P(0u, n_in) = A.cur;
        L.S(0u, n_in) = 0;
        ++n_in;
        pos_advance(A, c.pos, term);
      }
    }
    for (uint32_t t = 1; t + 1u < nt; ++t) {
      if (n_in == 0u) return 0u;
      uint32_t n_out = 0;
      if (!carry_fold(c, L, t, w, bit, slop, in, n_in, n_out)) {
        *over = true;
        return 0u;
      }
      in = 1u - in;
      n_in = n_out;
    }
    if (n_in == 0u) return 0u;
    return carry_last<COUNT>(c, L, nt - 1u, w, bit, slop, in, n_in);
  }
}

// the word of 32 docs that hold every list of the query and are alive
__device__ __forceinline__ uint32_t propose(const SlopCtx &c, const TqdSegment &seg, uint32_t nt, uint32_t w, bool in) {
  uint32_t match = in ? 0xFFFFFFFFu : 0u;
  for (uint32_t t = 0; t < nt; ++t) {
    const uint2 *bm = reinterpret_cast<const uint2 *>(c.tbase + ((uint64_t)sload(c.Q->dense_off + t) << 3));
    match &= in ? bm[w].x : 0u;
  }
  if (seg.alive) match &= in ? reinterpret_cast<const uint32_t *>(seg.alive)[w] : 0u;  // AliveBitSet
  return match;
}

#define TQ_SLOP_LDS(L, lane)                                  \
  Carry L{nullptr, nullptr, (uint32_t)(lane)};                \
  if constexpr (CARRY) {                                      \
    __shared__ uint32_t carry_pos[2u * CAP * 64u];            \
    __shared__ uint8_t carry_spent[2u * CAP * 64u];           \
    L.pos = carry_pos;                                        \
    L.sp = carry_spent;                                       \
  }

// ---- scoring: bm25(weight, norm, phrase count) into the per-tile top-k partials of the tree route
template <int KPL, bool CARRY>
__global__ __launch_bounds__(64) void phrase_slop_kernel(TqkPhraseSlopParams p) {
  const int lane = (int)__lane_id();
  const uint32_t q = blockIdx.x % p.n_queries, tile = blockIdx.x / p.n_queries;
  const TqdSlopQuery *Q = p.queries + q;
  const uint32_t nt = sload(&Q->n_terms);
  if (nt != 0u && (nt > 2u) != CARRY) return;  // (the other instantiation's query; an empty one is flushed by CARRY = false)
  if (nt == 0u && CARRY) return;
  const uint32_t k = sload(&Q->k), slop = sload(&Q->slop);
  const float weight = __uint_as_float(sload(&Q->weight_bits));
  const float *cache = p.caches + (size_t)sload(&Q->cache_idx) * 256u;
  const TqdSegment seg = p.seg;
  const SlopCtx c{Q, p.terms, p.table_base, seg.idx, seg.pos};
  TQ_SLOP_LDS(L, lane)
  TopK<KPL> tk;
  tk.reset(k);
  uint32_t n_matches = 0, n_over = 0;
  const uint32_t w_end = (tile + 1u) * TILE_WORDS < p.n_words ? (tile + 1u) * TILE_WORDS : p.n_words;
  for (uint32_t w0 = tile * TILE_WORDS; nt != 0u && w0 < w_end; w0 += 64u) {
    const uint32_t w = w0 + (uint32_t)lane;
    uint32_t rest = propose(c, seg, nt, w, w < w_end);
    while (__ballot(rest != 0u)) {  // every lane takes the lowest doc of its word until none has one left
      const bool has = rest != 0u;
      const uint32_t bit = has ? (uint32_t)__builtin_ctz(rest) : 0u;
      rest &= rest - 1u;
      const uint32_t doc = (w << 5) | bit;
      uint32_t cnt = 0;
      bool over = false;
      if (has) cnt = doc_verdict<true, CARRY>(c, L, nt, w, bit, slop, &over);
      n_over += over ? 1u : 0u;
      const bool ok = has && cnt > 0u;
      n_matches += ok ? 1u : 0u;
      const float s = ok ? bm25(weight, cache[fieldnorm_id(seg, doc)], cnt) : 0.0f;
      tk.offer(ok, make_key(s, doc), lane);
    }
  }
  flush_partial(tk, sload(&p.sinks->partials), sload(&Q->part_start) + tile, lane);
  for (int off = 32; off > 0; off >>= 1) {
    n_matches += __shfl_down(n_matches, off, 64);
    n_over += __shfl_down(n_over, off, 64);
  }
  if (lane == 0 && n_matches) {
    atomicAdd(sload(&p.sinks->query_matches) + sload(&p.sinks->out_index)[q], n_matches);
    atomicAdd(sload(&p.sinks->match_counter), (unsigned long long)n_matches);
  }
  if (CARRY && lane == 0 && n_over) atomicAdd(p.overflow + sload(&Q->out_q), n_over);
}

// ---- not scoring: the match bits of the query into its result bitmap of the doc-set batch's scratch, one writer per word
template <bool CARRY>
__global__ __launch_bounds__(64) void phrase_slop_bits_kernel(TqkPhraseSlopParams p) {
  const int lane = (int)__lane_id();
  const uint32_t q = blockIdx.x % p.n_queries, tile = blockIdx.x / p.n_queries;
  const TqdSlopQuery *Q = p.queries + q;
  const uint32_t nt = sload(&Q->n_terms);
  if (nt != 0u && (nt > 2u) != CARRY) return;
  if (nt == 0u && CARRY) return;
  const uint32_t slop = sload(&Q->slop);
  const TqdSegment seg = p.seg;
  const SlopCtx c{Q, p.terms, p.table_base, seg.idx, seg.pos};
  TQ_SLOP_LDS(L, lane)
  uint32_t *out = p.bits + (size_t)sload(&Q->part_start) * p.words_per_list;
  uint32_t n_over = 0;
  const uint32_t w_end = (tile + 1u) * TILE_WORDS < p.n_words ? (tile + 1u) * TILE_WORDS : p.n_words;
  for (uint32_t w0 = tile * TILE_WORDS; w0 < w_end; w0 += 64u) {
    const uint32_t w = w0 + (uint32_t)lane;
    const bool in = w < w_end;
    uint32_t match = nt ? propose(c, seg, nt, w, in) : 0u;
    uint32_t rest = match;
    while (rest != 0u) {  // (no cross-lane step in here: every lane walks its own word)
      const uint32_t bit = (uint32_t)__builtin_ctz(rest);
      rest &= rest - 1u;
      bool over = false;
      if (!doc_verdict<false, CARRY>(c, L, nt, w, bit, slop, &over)) match &= ~(1u << bit);
      n_over += over ? 1u : 0u;
    }
    if (in) out[w] = match;
  }
  if constexpr (CARRY) {
    for (int off = 32; off > 0; off >>= 1) n_over += __shfl_down(n_over, off, 64);
    if (lane == 0 && n_over) atomicAdd(p.overflow + sload(&Q->out_q), n_over);
  }
}

template <bool CARRY>
void launch_scored(const TqkPhraseSlopParams &p, int kpl, dim3 grid, dim3 block, hipStream_t st) {
  switch (kpl) {
    case 1: phrase_slop_kernel<1, CARRY><<<grid, block, 0, st>>>(p); break;
    case 2: phrase_slop_kernel<2, CARRY><<<grid, block, 0, st>>>(p); break;
    case 4: phrase_slop_kernel<4, CARRY><<<grid, block, 0, st>>>(p); break;
    default: phrase_slop_kernel<16, CARRY><<<grid, block, 0, st>>>(p); break;
  }
}

}  // namespace

// One launch per instantiation the group needs: the 2-list queries never run in a workgroup that holds the carried
// lists.  (pair: some query has 2 lists or is empty; carry: some query has 3 or more.)
hipError_t tqk_launch_phrase_slop(const TqkPhraseSlopParams &p, int kpl, hipStream_t st) {
  const uint32_t tiles = tqk_tree_tiles(p.n_words);
  if (!tiles || !p.n_queries) return hipSuccess;
  const dim3 grid(tiles * p.n_queries), block(64);
  if (p.any_pair) launch_scored<false>(p, kpl, grid, block, st);
  if (p.any_carry) launch_scored<true>(p, kpl, grid, block, st);
  return hipGetLastError();
}
hipError_t tqk_launch_phrase_slop_bits(const TqkPhraseSlopParams &p, hipStream_t st) {
  const uint32_t tiles = tqk_tree_tiles(p.n_words);
  if (!tiles || !p.n_queries) return hipSuccess;
  const dim3 grid(tiles * p.n_queries), block(64);
  if (p.any_pair) phrase_slop_bits_kernel<false><<<grid, block, 0, st>>>(p);
  if (p.any_carry) phrase_slop_bits_kernel<true><<<grid, block, 0, st>>>(p);
  return hipGetLastError();
}
