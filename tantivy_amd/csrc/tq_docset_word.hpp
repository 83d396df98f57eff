// tq_docset_word.hpp — the match bits of one query over bitmap words (the bitwise expression of a TqkDocsetQuery with
// the alive filter) and the wavefront prefix sum that turns them into positions.  Shared by tq_docset.hip (count /
// write passes) and tq_sort.hip (the selection of TopDocs::order_by_fast_field).  Internal linkage: every kernel file
// gets its own copy.
#pragma once
#include "tq_common.hpp"
#include "tq_launch.h"

namespace {

// Bit-sliced counter of one-bit-per-doc inputs saturating at 15, the SlicedCount of tq_tree.hip (kept in step with
// it by tests/test_gpu_docset.py's m-of-n shapes against the oracle): "at least m of the Should clauses", m <= 15.
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
  __device__ __forceinline__ uint32_t at_least(uint32_t m) const {  // m wave-uniform, 1..15
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

struct DocsetHead {  // the scalar part of a TqkDocsetQuery
  uint32_t n_terms, kinds, clause_end, should_end, narrow, min_should;
};

// The 32 result bits of bitmap word w (w < n_words) of one query: alive docs below max_doc only.
__device__ __forceinline__ uint32_t docset_word(const TqkDocsetQuery *Q, const DocsetHead &h, const TqkDocsetParams &p,
                                                uint32_t w) {
  uint32_t must = 0xFFFFFFFFu, nots = 0u, clause = 0u, any = 0u, sclause = 0u;
  SlicedCount sc;
  for (uint32_t m = 0; m < h.n_terms; ++m) {
    const uint32_t bits = ((h.narrow >> m) & 1u) ? reinterpret_cast<const uint32_t *>(Q->dense[m])[w] : Q->dense[m][w].x;
    const uint32_t kind = (h.kinds >> (2u * m)) & 3u;
    if (kind == TQK_COUNT_MUST) {
      clause |= bits;
      if ((h.clause_end >> m) & 1u) {
        must &= clause;
        clause = 0u;
      }
    } else if (kind == TQK_COUNT_NOT) {
      nots |= bits;
    } else {
      sclause |= bits;
      if ((h.should_end >> m) & 1u) {  // a Should clause (the OR of its lists) counts once
        any |= sclause;
        if (h.min_should >= 2u) sc.add(sclause);
        sclause = 0u;
      }
    }
  }
  uint32_t res = must & ~nots;
  if (h.min_should == 1u)
    res &= any;
  else if (h.min_should >= 2u)
    res &= sc.at_least(h.min_should);
  // AliveBitSet: bit d of byte d >> 3 (alive_bitset.rs:58-61) = bit d & 31 of little-endian word d >> 5
  if (p.alive) res &= reinterpret_cast<const uint32_t *>(p.alive)[w];
  // the segment's last word: an expression without Must lists is all ones there whatever the inputs hold
  if (w == p.n_words - 1u && (p.max_doc & 31u)) res &= (1u << (p.max_doc & 31u)) - 1u;
  return res;
}

__device__ __forceinline__ DocsetHead docset_head(const TqkDocsetQuery *Q) {
  DocsetHead h;
  h.n_terms = sload(&Q->n_terms);
  h.kinds = sload(&Q->kinds);
  h.clause_end = sload(&Q->clause_end);
  h.should_end = sload(&Q->should_end);
  h.narrow = sload(&Q->narrow);
  h.min_should = sload(&Q->min_should);
  return h;
}

__device__ __forceinline__ uint32_t wave_incl_sum(uint32_t v, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t u = __shfl_up(v, off, 64);
    if (lane >= off) v += u;
  }
  return v;
}

}  // namespace
