// tq_docset_score_fields.hip — docset_score_kernel (tq_docset_score.hip) over scoring lists of SEVERAL fields of a
// multi-field segment (tq_fields.cpp): the same access paths, the same sums in the same association — list m scores
// under the norm of ITS field.  A duplicate of tq_docset_score.hip's kernel, so that the single-field instantiations
// stay the code they were; read that file for the pass itself.  What differs: the field of list m rides in bits 8..10 of
// TqkScoreQuery::shift[m] (scalar loads), the fieldnorm pointers of fields 1.. in the launch parameters
// (TqkScoreFieldsParams), and the doc's fieldnorm bytes of the query's fields are gathered right behind the doc itself,
// in front of the chunks of lists (tq_fields.h).  HBM model per output doc: 4 (doc) + 4 (score) + one fieldnorm byte per
// field the query names.
#include "tq_common.hpp"
#include "tq_launch.h"
#include "tq_fields.h"

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
__global__ __launch_bounds__(SC_THREADS) void docset_score_fields_kernel(TqkScoreFieldsParams pp) {
  const TqkScoreParams &p = pp.base;
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
  uint32_t fmask = 0u;  // the fields the query's scoring lists belong to
  for (uint32_t m = 0; m < n_lists; ++m) fmask |= 1u << ((sload(&Q->shift[m]) >> 8) & 7u);
  for (uint32_t base = (threadIdx.x & ~63u); base < n; base += SC_THREADS) {  // (uniform for the wavefront)
    const uint32_t j = base + (uint32_t)lane;
    uint32_t doc = 0;
    bool on = j < n;
    if (on) doc = p.out_docs[start + j];
    on = on && doc < seg.max_doc;
    TQ_FIELD_NORMS(cache, fmask, seg.fieldnorm, pp.fn, seg.const_fieldnorm_id, on, doc);
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
          present = rdir_lookup(dir, ent, sload(&Q->shift[m]) & 0xFFu, doc, on, tf, pi);
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
        if (present) clause = clause + (kind == TQK_SCORE_CONST ? w : bm25(w, TQ_FIELD_NORM_OF((sload(&Q->shift[m]) >> 8) & 7u), tf));
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

hipError_t tqk_launch_docset_score_fields(const TqkScoreFieldsParams &p, hipStream_t st) {
  if (!p.base.n_tiles || !p.base.n_queries) return hipSuccess;
  if (p.base.any_blocks)
    docset_score_fields_kernel<true><<<dim3(p.base.n_tiles * p.base.n_queries), dim3(SC_THREADS), 0, st>>>(p);
  else
    docset_score_fields_kernel<false><<<dim3(p.base.n_tiles * p.base.n_queries), dim3(SC_THREADS), 0, st>>>(p);
  return hipGetLastError();
}
