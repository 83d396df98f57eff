// Scores of full doc sets (Weight::for_each -> for_each_scorer, src/query/weight.rs:9-18,89-97: what a collector whose
// requires_scoring() is true gets from default_collect_segment_impl, src/collector/mod.rs:186-221): the pass behind
// tq_docset.hip's write pass.  The rows are there already — alive docs, ascending, at tile_offs — so this pass only
// asks every scoring list of the query "is doc d in the list, with which tf" and adds the BM25 terms up in the
// unpruned scorers' order:
//   Must clauses, cheapest first     Intersection::score = first + second + (0 + the others) (intersection.rs:325-329)
//   a clause of several lists        the sum of its present lists in clause order, from 0 (SumCombiner)
//   Should clauses                   opt = the sum of the present clauses from 0; beside a Must part req + opt
//                                    (reqopt_scorer.rs:85-98), alone the union's score
// Workgroup = (query, tile of 65 536 docs), query fastest, as the count and write passes; consecutive lanes take
// consecutive output positions of the tile: out_docs is read and out_scores written coalesced, the fieldnorm byte and
// every list's bitmap word are gathered from addresses that ascend with the lane.  One lane computes one doc's score
// in that fixed association: no atomics, nothing that depends on the order of lanes.
// A list is reached through its bitmap + rank directory and byte-wide tfs, through its range directory, or — the general
// case, in an instantiation of its own because of the LDS it needs — by seek_block + lookup_in_blocks; a saturated tf
// byte (255) or directory entry (0xFFFF) reads the packed value of the posting's block.  The batch's scratch bitmaps
// are not read: they belong to whichever sub-batch ran last.  A TERM SET (tq_termset.cpp) is the fourth kind: its bitmap
// word says whether the doc is in it, and it scores the query's weight as given (ConstScorer) — no rank, no tf, no norm.
// HBM model per output doc: 4 (doc) + 4 (score) + 1 (fieldnorm) bytes; per scoring list at most one 8-byte bitmap
// word per 32 docs of the segment.
#include "tq_common.hpp"
#include "tq_launch.h"

namespace {

constexpr uint32_t SC_THREADS = 256;
constexpr uint32_t SC_WAVES = SC_THREADS / 64;
#ifndef TQ_SCORE_CHUNK
#define TQ_SCORE_CHUNK 4
#endif
constexpr uint32_t SC_CHUNK = TQ_SCORE_CHUNK;  // lists whose gathers are in flight together

template <bool BLOCKS>
struct ScoreLds {
  uint32_t pay[SC_WAVES][520];  // lookup_in_blocks: four 512-byte regions + a spare row, per wavefront
};
template <>
struct ScoreLds<false> {};

// the packed tf of posting pi of a list (a saturated byte or directory entry; a list without tf bytes)
__device__ __forceinline__ uint32_t exact_tf(const uint8_t *idx, const TermRef &tr, uint32_t pi) {
  const uint4 r = tr.rec[pi >> 7];
  return block_tf_at(idx, tr, make_uint2(r.y, r.z), pi & 127u);
}

template <bool BLOCKS>
__global__ __launch_bounds__(SC_THREADS) void docset_score_kernel(TqkScoreParams p) {
  __shared__ __attribute__((aligned(16))) ScoreLds<BLOCKS> L;
  const int lane = (int)__lane_id();
  const uint32_t q = blockIdx.x % p.n_queries, tile = blockIdx.x / p.n_queries;
  const size_t entry = (size_t)q * p.n_tiles + tile;
  const uint32_t tile_docs = p.tile_counts[entry];
  if (tile_docs == 0u) return;  // (uniform for the workgroup)
  const uint64_t start = p.tile_offs[entry];
  if (start >= p.out_cap) return;  // nothing of this tile was written
  const uint32_t n = (uint32_t)(p.out_cap - start < (uint64_t)tile_docs ? p.out_cap - start : (uint64_t)tile_docs);
  const TqkScoreQuery *Q = p.queries + q;
  const uint32_t n_lists = sload(&Q->n_lists), access = sload(&Q->access), clause_end = sload(&Q->clause_end);
  const uint32_t n_must_lists = sload(&Q->n_must_lists), all_base_bits = sload(&Q->all_base_bits);
  const float *cache = p.caches + (size_t)sload(&Q->cache_idx) * 256u;
  const TqdSegment &seg = p.seg;
  for (uint32_t base = (threadIdx.x & ~63u); base < n; base += SC_THREADS) {  // (uniform for the wavefront)
    const uint32_t j = base + (uint32_t)lane;
    uint32_t doc = 0;
    bool on = j < n;
    if (on) doc = p.out_docs[start + j];
    on = on && doc < seg.max_doc;
    const float norm = cache[on ? fieldnorm_id(seg, doc) : 0u];
    const uint32_t bit = doc & 31u;
    float first = 0.0f, second = 0.0f, others = 0.0f, opt = 0.0f, clause = 0.0f;
    uint32_t n_must = 0;
    // The pass is bound by gather latency, not by bytes: asked one after the other, a list's bitmap word and then its tf
    // byte are two dependent round trips per list and doc.  So the lists are taken SC_CHUNK at a time: every bitmap
    // word of the chunk is requested first, then every tf byte, and only then are the terms added up, in list order.
    for (uint32_t m0 = 0; m0 < n_lists; m0 += SC_CHUNK) {
      uint2 wd[SC_CHUNK];
      uint32_t tfb[SC_CHUNK];
#pragma unroll
      for (uint32_t u = 0; u < SC_CHUNK; ++u) {
        const uint32_t m = m0 + u;
        wd[u] = make_uint2(0u, 0u);
        const uint32_t kind_u = (access >> (2u * m)) & 3u;
        if (m < n_lists && (kind_u == TQK_SCORE_BITMAP || kind_u == TQK_SCORE_CONST)) {  // (uniform)
          const uint2 *bm = reinterpret_cast<const uint2 *>(sload(reinterpret_cast<const uint64_t *>(Q->tab) + m));
          if (on) wd[u] = bm[doc >> 5];
        }
      }
#pragma unroll
      for (uint32_t u = 0; u < SC_CHUNK; ++u) {
        const uint32_t m = m0 + u;
        tfb[u] = 255u;
        if (m < n_lists && ((access >> (2u * m)) & 3u) == TQK_SCORE_BITMAP) {
          const uint8_t *tf8 = reinterpret_cast<const uint8_t *>(sload(reinterpret_cast<const uint64_t *>(Q->aux) + m));
          if (((wd[u].x >> bit) & 1u) && tf8) tfb[u] = tf8[wd[u].y + (uint32_t)__popc(wd[u].x & ((1u << bit) - 1u))];
        }
      }
#pragma unroll
      for (uint32_t u = 0; u < SC_CHUNK; ++u) {
        const uint32_t m = m0 + u;
        if (m >= n_lists) break;
        const uint32_t kind = (access >> (2u * m)) & 3u;
        const float w = __uint_as_float(sload(reinterpret_cast<const uint32_t *>(Q->weight) + m));
        bool present = false;
        uint32_t tf = 1u;
        if (kind == TQK_SCORE_BITMAP) {
          present = (wd[u].x >> bit) & 1u;
          tf = tfb[u];
          if (__ballot(present && tf == 255u)) {  // saturated (or no tf bytes): the packed value
            const TermRef tr = load_term(p.terms, sload(&Q->handle[m]));
            if (present && tf == 255u) tf = exact_tf(seg.idx, tr, wd[u].y + (uint32_t)__popc(wd[u].x & ((1u << bit) - 1u)));
          }
        } else if (kind == TQK_SCORE_RDIR) {
          const uint32_t *dir = reinterpret_cast<const uint32_t *>(sload(reinterpret_cast<const uint64_t *>(Q->tab) + m));
          const uint32_t *ent = reinterpret_cast<const uint32_t *>(sload(reinterpret_cast<const uint64_t *>(Q->aux) + m));
          uint32_t pi = 0;
          present = rdir_lookup(dir, ent, sload(&Q->shift[m]), doc, on, tf, pi);
          if (__ballot(present && tf == 0xFFFFu)) {
            const TermRef tr = load_term(p.terms, sload(&Q->handle[m]));
            if (present && tf == 0xFFFFu) tf = exact_tf(seg.idx, tr, pi);
          }
        } else if (kind == TQK_SCORE_CONST) {  // a term set: the bit alone
          present = (wd[u].x >> bit) & 1u;
        } else if constexpr (BLOCKS) {  // (TQK_SCORE_BLOCKS: the kinds above are tested explicitly)
          const TermRef tr = load_term(p.terms, sload(&Q->handle[m]));
          bool cand = on;
          uint32_t jb = 0;
          if (cand) {
            jb = seek_block(tr, doc);
            cand = jb < tr.n_blocks;
          }
          uint32_t unused;
          const uint32_t at = lookup_in_blocks<false>(seg.idx, tr, jb, doc, cand, L.pay[threadIdx.x >> 6], lane, &unused);
          present = cand && at != NOT_FOUND;
          if (present) {
            const uint4 r = tr.rec[jb];
            tf = block_tf_at(seg.idx, tr, make_uint2(r.y, r.z), at);
          }
        }
        if (present) clause = clause + (kind == TQK_SCORE_CONST ? w : bm25(w, norm, tf));
        if ((clause_end >> m) & 1u) {  // (uniform)
          if (m < n_must_lists) {
            if (n_must == 0u)
              first = clause;
            else if (n_must == 1u)
              second = clause;
            else
              others = others + clause;
            ++n_must;
          } else {
            opt = opt + clause;
          }
          clause = 0.0f;
        }
      }
    }
    float s = n_must == 0u ? opt : (n_must == 1u ? first : (first + second) + others);
    if (n_must != 0u && n_lists > n_must_lists) s = s + opt;
    // an ALL-BASED query: the AllScorer's share comes last (fl32(s + base)); alone it is the score
    if (all_base_bits) s = n_lists ? s + __uint_as_float(all_base_bits) : __uint_as_float(all_base_bits);
    if (on) p.out_scores[start + j] = s;
  }
}

}  // namespace

hipError_t tqk_launch_docset_score(const TqkScoreParams &p, hipStream_t st) {
  if (!p.n_tiles || !p.n_queries) return hipSuccess;
  if (p.any_blocks)
    docset_score_kernel<true><<<dim3(p.n_tiles * p.n_queries), dim3(SC_THREADS), 0, st>>>(p);
  else
    docset_score_kernel<false><<<dim3(p.n_tiles * p.n_queries), dim3(SC_THREADS), 0, st>>>(p);
  return hipGetLastError();
}
