// tq_all.hip — top-k of ALL-BASED queries: flat queries whose AllQuery clauses (TQ_TERM_ALL, src/query/all_query.rs:23-112)
// make every doc of the segment a candidate — `*`, `+* -spam`, `+* a b`, `* a b` (tq_all.cpp has the normal form,
// BooleanWeight::complex_scorer read literally: boolean_weight.rs:114-171, 236-431).  The doc set is every alive doc
// (or the docs that hold at least m' of the Should clauses) minus the MustNot lists; a doc scores the f32 sum of its
// present Should clauses (0 + the lists in query order, a clause_of union summed inside the clause first) + base, the
// one AllScorer's 1.0 (RequiredOptionalScorer / Intersection / SumCombiner all add it once), or the sole All's boost.
//
// One wavefront per (query, tile of TQK_ALL_TILE_WORDS = 2 048 bitmap words = 65 536 docs), query fastest as in
// tree_kernel; a lane owns one 32-doc word per step: one coalesced 8-byte load per list per step, descriptors read
// wave-uniformly.  Nearly every doc matches, so the work per match has to be close to nothing for the docs that score
// only the base:
//   scored = set & (any Should list)   bitmap word -> rank -> tf byte per present list, BM25 with the IEEE divide, the
//                                      per-wave top-k in registers (what tree_kernel does for a matching doc);
//   set & ~scored (m' == 0 only)       they all score exactly `base` and ties go to the lower doc: a tile offers its
//                                      FIRST k of them in doc order — a wave-wide prefix sum of popcounts picks them —
//                                      and none once the k-th key of the wave is above (base, first remaining doc).
//                                      The rest is skipped by a popcount: `+* a b` does not insert 65 536 docs per tile.
// Nothing is pruned (the reference runs these shapes through for_each_pruning_scorer, weight.rs:47-60): "exhaustive"
// 0 and 1 give the same rows, and the match count is the size of the doc set, from popcounts.  A query without lists
// on a segment without deletes scans only its ceil(k / 65 536) first tiles; the docs of the others are counted by the
// planner (extra_matches).  Partial lists go through merge_kernel like every per-tile group's.
//
// HBM model: per scanned tile 8 B per list per 32 docs (4 would do for a MustNot list: the rank half of its words
// rides along) + 4 B of alive bits per 32 docs; per scored doc 1 fieldnorm byte + 1 tf byte per present list.
#include "tq_common.hpp"
#include "tq_launch.h"

namespace {

// "at least m of the Should clauses", m <= 15: the SlicedCount of tq_tree.hip / tq_docset.hip (saturating at 15)
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

__device__ __forceinline__ uint32_t wave_incl_sum(uint32_t v, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t u = __shfl_up(v, off, 64);
    if (lane >= off) v += u;
  }
  return v;
}

template <int KPL>
__global__ __launch_bounds__(64) void all_kernel(TqkAllParams p) {
  const int lane = (int)__lane_id();
  const uint32_t q = blockIdx.x % p.n_queries, tile = blockIdx.x / p.n_queries;
  const TqdAllQuery *Q = p.queries + q;
  if (tile >= sload(&Q->n_tiles)) return;  // (the query scans fewer tiles than the launch's largest: no list of its own here)
  const uint32_t nl = sload(&Q->n_lists), ns = sload(&Q->n_should), k = sload(&Q->k);
  const uint32_t clause_end = sload(&Q->clause_end), need = sload(&Q->min_should);
  const float base = __uint_as_float(sload(&Q->base_bits));
  const float *cache = p.caches + (size_t)sload(&Q->cache_idx) * 256u;
  const uint8_t *tbase = p.table_base;
  const TqdSegment seg = p.seg;
  TopK<KPL> tk;
  tk.reset(k);
  uint32_t n_matches = 0, n_scored = 0;  // the doc set's size; the docs whose BM25 was evaluated
  uint32_t base_left = k;  // base-only docs this tile may still offer (wave-uniform)
  const uint32_t w_end = (tile + 1u) * TQK_ALL_TILE_WORDS < p.n_words ? (tile + 1u) * TQK_ALL_TILE_WORDS : p.n_words;
  for (uint32_t w0 = tile * TQK_ALL_TILE_WORDS; w0 < w_end; w0 += 64u) {
    const uint32_t w = w0 + (uint32_t)lane;
    const bool in = w < w_end;
    // ---- the doc set of 32 docs per lane
    uint32_t nots = 0u, any = 0u, clause = 0u;
    SlicedCount sc;
    for (uint32_t t = 0; t < nl; ++t) {
      const uint2 *bm = reinterpret_cast<const uint2 *>(tbase + ((uint64_t)sload(Q->dense_off + t) << 3));
      const uint32_t bits = in ? bm[w].x : 0u;
      if (t < ns) {
        clause |= bits;
        if ((clause_end >> t) & 1u) {  // a Should clause (the OR of its lists) counts once
          any |= clause;
          if (need >= 2u) sc.add(clause);
          clause = 0u;
        }
      } else {
        nots |= bits;
      }
    }
    uint32_t set = in ? ~nots : 0u;
    if (seg.alive) set &= in ? reinterpret_cast<const uint32_t *>(seg.alive)[w] : 0u;  // AliveBitSet (alive_bitset.rs:58-61)
    // the segment's last word: without a Must list the expression is all ones there whatever the inputs hold
    if (w == p.n_words - 1u && (seg.max_doc & 31u)) set &= (1u << (seg.max_doc & 31u)) - 1u;
    if (need == 1u)
      set &= any;
    else if (need >= 2u)
      set &= sc.at_least(need);
    n_matches += (uint32_t)__popc(set);
    const uint32_t scored = set & any;
    n_scored += (uint32_t)__popc(scored);
    // ---- the docs that score only the base: the tile's first k in doc order, none once they cannot enter the top-k
    uint32_t only = set & ~scored;
    if (base_left && tk.thr > make_key(base, w0 << 5)) base_left = 0u;  // (every doc from here on has a smaller key)
    if (base_left == 0u) only = 0u;
    if (__ballot(only != 0u)) {
      const uint32_t cnt = (uint32_t)__popc(only);
      const uint32_t incl = wave_incl_sum(cnt, lane);
      const uint32_t before = incl - cnt, total = (uint32_t)__shfl(incl, 63, 64);
      const uint32_t room = base_left > before ? base_left - before : 0u;
      if (cnt > room) {  // (the lane where the tile's k-th base-only doc falls, and the lanes behind it)
        uint32_t kept = 0u, r = only;
        for (uint32_t i = 0; i < room; ++i) {
          kept |= r & (0u - r);
          r &= r - 1u;
        }
        only = kept;
      }
      base_left -= total < base_left ? total : base_left;
    }
    // ---- score and offer: every lane takes the lowest doc of its word until none has one left
    uint32_t todo = scored | only;
    while (__ballot(todo != 0u)) {
      const bool has = todo != 0u;
      const uint32_t bit = has ? (uint32_t)__builtin_ctz(todo) : 0u;
      todo &= todo - 1u;
      const uint32_t doc = (w << 5) | bit;
      float s = 0.0f, csum = 0.0f;
      if (__ballot(has && ((scored >> bit) & 1u))) {  // (a round of base-only docs reads no list)
        const float norm = cache[has ? fieldnorm_id(seg, doc) : 0u];
        for (uint32_t t = 0; t < ns; ++t) {
          const uint2 *bm = reinterpret_cast<const uint2 *>(tbase + ((uint64_t)sload(Q->dense_off + t) << 3));
          uint2 wd = make_uint2(0u, 0u);
          if (has) wd = bm[w];
          if (has && ((wd.x >> bit) & 1u)) {
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
            csum = csum + bm25(__uint_as_float(sload(Q->weight_bits + t)), norm, tf);
          }
          if ((clause_end >> t) & 1u) {  // SumCombiner: the clause's sum joins the Should sum
            s = s + csum;
            csum = 0.0f;
          }
        }
      }
      s = ns ? s + base : base;  // the AllScorer's share comes last; a doc no Should list holds scores the base
      tk.offer(has, make_key(s, doc), lane);
    }
  }
  flush_partial(tk, sload(&p.sinks->partials), sload(&Q->part_start) + tile, lane);
  for (int off = 32; off > 0; off >>= 1) {
    n_matches += __shfl_down(n_matches, off, 64);
    n_scored += __shfl_down(n_scored, off, 64);
  }
  if (lane == 0) {
    // per query: the size of the doc set (tq_last_batch_match_counts = what tq_count_batch gives); for the batch's
    // statistics: the docs that read a fieldnorm byte and tf bytes (a base-only doc reads nothing)
    if (tile == 0u) n_matches += sload(&Q->extra_matches);
    if (n_matches) atomicAdd(sload(&p.sinks->query_matches) + sload(&p.sinks->out_index)[q], n_matches);
    if (n_scored) atomicAdd(sload(&p.sinks->match_counter), (unsigned long long)n_scored);
  }
}

}  // namespace

uint32_t tqk_all_tiles(uint32_t n_words) { return (n_words + TQK_ALL_TILE_WORDS - 1u) / TQK_ALL_TILE_WORDS; }

hipError_t tqk_launch_all(const TqkAllParams &p, int kpl, hipStream_t st) {
  if (!p.max_tiles || !p.n_queries) return hipSuccess;
  const dim3 grid(p.max_tiles * p.n_queries), block(64);
  switch (kpl) {
    case 1: all_kernel<1><<<grid, block, 0, st>>>(p); break;
    case 2: all_kernel<2><<<grid, block, 0, st>>>(p); break;
    case 4: all_kernel<4><<<grid, block, 0, st>>>(p); break;
    default: all_kernel<16><<<grid, block, 0, st>>>(p); break;
  }
  return hipGetLastError();
}
