// tq_docset_walk.hpp — the walk of one query's match bits that hands every matching doc to a lane: the loop of the
// kernels that consume a doc set without writing it (tq_sort.hip, tq_agg.hip, tq_agg_sub.hip, tq_agg_terms.hip,
// tq_agg_terms_sub.hip, tq_agg_range.hip, tq_agg_terms_hist.hip).  A workgroup = (query, slice of the bitmap words) of four wavefronts, each walking every fourth
// 64-word chunk of the slice on its own (no workgroup barrier inside the walk):
//   1. a lane evaluates one word (docset_word, tq_docset_word.hpp), the popcounts are prefix-summed over the wavefront
//   2. every lane expands its word's bits into the wavefront's LDS slab (13 bits per doc: word of the chunk, bit)
//   3. the slab is read back 64 docs a round — a lane per matching doc, whatever the words' densities — and the round is
//      handed to the caller
// tq_docset.hip's write pass is not this loop (its slab is indexed by the workgroup's thread).  Internal linkage, like
// tq_docset_word.hpp: every kernel file gets its own copy.
#pragma once
#include "tq_common.hpp"
#include "tq_docset_word.hpp"
#include "tq_launch.h"

namespace {

constexpr uint32_t WALK_THREADS = 256;
constexpr uint32_t WALK_WAVES = WALK_THREADS / 64;
constexpr uint32_t WALK_CHUNK_WORDS = 64;                          // one word per lane
constexpr uint32_t WALK_CHUNK_DOCS = WALK_CHUNK_WORDS * 32;        // slab entries per wavefront
constexpr uint32_t WALK_STEP_WORDS = WALK_WAVES * WALK_CHUNK_WORDS;  // bitmap words a workgroup takes per step
constexpr uint32_t WALK_SLAB_ENTRIES = WALK_WAVES * WALK_CHUNK_DOCS;  // uint16_t each: 16 KB of LDS

// Walks words [slice * words_per_slice, (slice + 1) * words_per_slice) of query Q, clamped to ds.n_words (a slice past the
// end: empty).  `slabs` is the workgroup's WALK_SLAB_ENTRIES entries of LDS.  per_doc(has, doc) is called by ALL 64 lanes
// of the wavefront on every round — converged, so it may ballot and shuffle; a lane without a doc of the round has
// has == false and an in-range doc it must not count.  Returns the lane's sum of popcounts: reduced over the wavefronts
// it is the slice's match count.
template <class PerDoc>
__device__ __forceinline__ uint32_t docset_walk(const TqkDocsetParams &ds, const TqkDocsetQuery *Q, uint32_t slice,
                                                uint32_t words_per_slice, uint16_t *slabs, uint32_t wave, int lane,
                                                PerDoc &&per_doc) {
  const DocsetHead h = docset_head(Q);
  uint16_t *const slab = slabs + wave * WALK_CHUNK_DOCS;
  const uint64_t w0_64 = (uint64_t)slice * words_per_slice;
  const uint64_t w1_64 = w0_64 + words_per_slice;
  const uint32_t w0 = w0_64 < ds.n_words ? (uint32_t)w0_64 : ds.n_words;
  const uint32_t w1 = w1_64 < ds.n_words ? (uint32_t)w1_64 : ds.n_words;
  uint32_t cnt = 0;
  for (uint32_t base = w0 + wave * WALK_CHUNK_WORDS; base < w1; base += WALK_STEP_WORDS) {
    const uint32_t w = base + (uint32_t)lane;
    uint32_t res = w < w1 ? docset_word(Q, h, ds, w) : 0u;
    const uint32_t pc = (uint32_t)__popc(res);
    cnt += pc;
    const uint32_t incl = wave_incl_sum(pc, lane);
    const uint32_t total = (uint32_t)__shfl(incl, 63, 64);  // <= WALK_CHUNK_DOCS
    uint32_t at = incl - pc;
    while (res) {
      slab[at++] = (uint16_t)(((uint32_t)lane << 5) | (uint32_t)__builtin_ctz(res));
      res &= res - 1u;
    }
    wave_mem_fence();
    for (uint32_t j = 0; j < total; j += 64u) {
      const bool has = j + (uint32_t)lane < total;
      const uint32_t e = has ? slab[j + (uint32_t)lane] : 0u;
      per_doc(has, ((base + (e >> 5)) << 5) | (e & 31u));
    }
    wave_mem_fence();  // (the next chunk's expansion writes the slab again)
  }
  return cnt;
}

}  // namespace
